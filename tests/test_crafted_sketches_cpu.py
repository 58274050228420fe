"""No GPU: the helpers behind the crafted sketch, metrics and partition tests are pinned to the library and the oracle, the planted
streams reach their branches (on the oracle's arrays), and the HyperLogLog estimate — the library's and the oracle's — is checked
against exact rational arithmetic on the registers that crafted addresses produce."""
import ctypes as C
import math

import numpy as np
import pytest

import keycraft as kc
import sketchcraft as sc


# ---------------------------------------------------------------- addresses
def test_ip_hash_restatement_and_crafted_addresses_match_library_and_oracle(nf, O):
    rng = np.random.default_rng(21)
    addrs = rng.integers(0, 256, size=(1000, 16), dtype=np.uint8)
    lo, hi = kc.ip_words(addrs)
    edge = np.array([0, 1, 1 << 63, kc.M64], dtype=np.uint64)
    for seed in range(4):
        mine = kc.ip_hash(lo, hi, seed)
        for a, h in zip(addrs, mine.tolist()):
            assert nf.ip_hash(a.tobytes(), seed) == O.lib().orc_ip_hash(a.tobytes(), seed) == h
        targets = np.concatenate([edge, edge, rng.integers(0, 1 << 64, size=50, dtype=np.uint64)])       # every edge hash twice: two addresses
        made = kc.craft_ip(targets, seed, rng)
        assert made.shape == (len(targets), 16) and made.dtype == np.uint8 and len(np.unique(made, axis=0)) == len(made)
        for a, t in zip(made, targets.tolist()):
            assert nf.ip_hash(a.tobytes(), seed) == O.lib().orc_ip_hash(a.tobytes(), seed) == t


@pytest.mark.parametrize("p", [4, 10, 14, 18])
def test_hll_targets_give_the_register_and_rho_asked_for(O, p):
    rng = np.random.default_rng(p)
    top = sc.max_rho(p)
    regs = np.concatenate([[0, (1 << p) - 1], rng.integers(0, 1 << p, size=top - 2)])
    rhos = np.arange(1, top + 1)
    h = sc.hll_targets(p, regs, rhos, rng)
    assert sc.rho_of(h, p) == list(zip(regs.tolist(), rhos.tolist()))
    addrs = kc.craft_ip(h, sc.HLL_SEED, rng)
    want = np.zeros(1 << p, dtype=np.uint8)
    np.maximum.at(want, regs, rhos.astype(np.uint8))
    got = np.zeros(1 << p, dtype=np.uint8)
    for a in addrs:                                                                       # the oracle's own update agrees with rho_of
        O.lib().orc_hll_update(got.ctypes.data_as(C.c_void_p), p, a.tobytes())
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- the planted streams reach their branches
@pytest.fixture(scope="module")
def planted(O):
    return sc.planted_streams(O)


@pytest.mark.parametrize("p,depth,log2w", sc.CONFIGS)
def test_planted_streams_reach_their_branches(O, planted, p, depth, log2w):
    recs, info, sk = planted[p]
    sc.check_preconditions(O, p, log2w, sk, info)
    assert len(recs) == sc.N_RECORDS + 256 and info["flows"] > 4000
    lo, hi = kc.ip_words(info["cm_first"])
    assert not (kc.ip_hash(lo, hi, sc.CM_SEED) >> np.uint64(64 - log2w)).any()
    lo, hi = kc.ip_words(info["cm_last"])
    assert ((kc.ip_hash(lo, hi, sc.CM_SEED) >> np.uint64(64 - log2w)) == (1 << log2w) - 1).all()
    # the block at the head: every wave of 64 records holds the four registers of one word, 16 times each
    lo, hi = kc.ip_words(recs.view(np.uint8).reshape(len(recs), 144)[:256, 16:32])
    regs = (kc.ip_hash(lo, hi, sc.HLL_SEED) >> np.uint64(64 - p)).astype(np.int64).reshape(4, 64)
    for wave in regs:
        assert np.array_equal(np.bincount(wave - 4 * info["word"], minlength=4), [16] * 4)
    by = recs["metrics"]["bytes"]                                                          # the byte edges are there, and variant 1's large counts too
    assert set(sc.EDGE_BYTES.tolist()) <= set(by.tolist())
    # rising and falling ladders: first records' rho per register, in arrival order over the whole stream, its head included
    raw = recs.view(np.uint8).reshape(len(recs), 144)
    lad = {a.tobytes() for a in info["rho_ladder"]}
    assert not any(raw[i, :16].tobytes() in lad for i in range(256)), "the block at the head brings no ladder address forward"
    seen, order = set(), {}
    for i in range(len(raw)):
        a = raw[i, :16].tobytes()
        if a in lad and a not in seen:
            seen.add(a)
            (reg, rho), = sc.rho_of(kc.ip_hash(*kc.ip_words(raw[i, :16]), sc.HLL_SEED), p)
            order.setdefault(reg, []).append(rho)
    top = sc.max_rho(p)
    kinds = sorted((v == list(range(1, top + 1))) - (v == list(range(top, 0, -1))) for v in order.values())
    assert len(order) == 16 and kinds == [-1] * 8 + [1] * 8, "eight registers with rising rho, eight with falling"


# ---------------------------------------------------------------- the estimate against exact arithmetic
def check_estimate(nf, O, what, p, regs):
    """<= 2 ULP from the exact value (the sum is exact and rounded once, alpha m^2 is exact, the division rounds once), and the
    library and the oracle bit for bit. Returns the figures."""
    exact, gap = sc.exact_hll_estimate(regs, p)
    assert gap > 2, "%s: the raw estimate is within 2 ULP of the branch point 2.5 m: choose another input" % what
    hist = np.bincount(regs, minlength=65).astype(np.uint32)
    lib, orc = nf.hll_estimate_from_histogram(hist, p), O.hll_estimate(regs, p)
    print("%s: exact %r library %r (%.1f ULP) oracle %r (%.1f ULP)" % (what, exact, lib, sc.ulps(lib, exact), orc, sc.ulps(orc, exact)))
    assert sc.ulps(orc, exact) <= 2, what
    assert sc.ulps(lib, exact) <= 2, what
    assert lib == orc, what
    return exact, lib, orc


def test_estimate_against_exact_arithmetic(nf, O, planted):
    """The exact reference: sum = sum_k hist[k] 2^(64 - k) as an integer, e = Fraction(alpha) m^2 2^64 / sum rounded once, the
    small-range branch as the same double expression.

    Before orc_hll_estimate accumulated its sum exactly it added 2^-reg register by register in doubles: on half_half (p = 18,
    2^17 registers at 1, then 2^17 at 47) every 2^-47 fell below half an ULP of the running sum 2^16 and was lost, and the
    oracle ended 92 ULP from the exact value; the library's 65 histogram terms were 0 ULP from it. On a ladder of all rho at
    p = 10 both were 1 ULP off."""
    for p, n, regs in sc.seeded_registers():
        check_estimate(nf, O, "seeded p=%d n=%d" % (p, n), p, regs)
    for p, (_, _, sk) in planted.items():
        check_estimate(nf, O, "planted p=%d src" % p, p, sk[2])
        check_estimate(nf, O, "planted p=%d dst" % p, p, sk[3])
    check_estimate(nf, O, "half_half", 18, sc.half_half_registers())
    ladder = np.zeros(1 << 10, dtype=np.uint8)
    ladder[:55] = np.arange(1, 56)
    check_estimate(nf, O, "one ladder, p=10", 10, ladder)
    check_estimate(nf, O, "all registers at 61, p=4", 4, np.full(16, 61, dtype=np.uint8))
    assert nf.hll_estimate_from_histogram(np.bincount(np.zeros(16, dtype=np.uint8), minlength=65).astype(np.uint32), 4) == 0.0 == O.hll_estimate(np.zeros(16, dtype=np.uint8), 4)


def test_half_half_stream_gives_the_half_half_registers(O):
    recs = sc.half_half_stream(O)
    assert kc.distinct_flows(recs) == len(recs) == 1 << 18
    _, _, hs, _ = O.sketches(recs, 1, 4, 18)
    assert np.array_equal(hs, sc.half_half_registers())


def test_exact_reference_takes_the_small_range_branch_like_the_code():
    regs = np.zeros(1 << 14, dtype=np.uint8)
    regs[:100] = 3
    e, gap = sc.exact_hll_estimate(regs, 14)
    assert e == float(1 << 14) * math.log(float(1 << 14) / float((1 << 14) - 100)) and gap > 2
    assert sc.exact_hll_estimate(np.full(16, 1, dtype=np.uint8), 4) == (0.673 * 16 * 16 / 8.0, math.inf)


# ---------------------------------------------------------------- the metrics fold's group hash, the constants
def test_metrics_group_hash_restatement_matches_the_library(nf):
    rng = np.random.default_rng(5)
    n = 10_000
    g = np.zeros(n + 1, dtype=nf.METRIC_GROUP)
    g["src_class"][:n], g["dst_class"][:n] = rng.integers(0, 1 << 22, n), rng.integers(0, 1 << 22, n)
    g["src_label"][:n], g["dst_label"][:n] = rng.integers(0, 1 << 16, n), rng.integers(0, 1 << 16, n)
    g["direction"][:n], g["layer"][:n], g["proto"][:n], g["is_ip"][:n] = rng.integers(0, 256, n), rng.integers(0, 3, n), rng.integers(0, 256, n), rng.integers(0, 2, n)
    g["src_label"][n], g["dst_label"][n], g["direction"][n] = nf._lib.NET_NO_LABEL, nf._lib.NET_NO_LABEL, nf._lib.NET_NO_DIRECTION      # the all-"none" key
    g["flows"], g["bytes"], g["pad_"] = 7, rng.integers(0, 1 << 60, n + 1), 9                   # not part of the key
    for grouping in (0, 3, 7):
        want = nf.metrics_group_hash(grouping, g)
        got = kc.metrics_group_hash(grouping, *(g[f] for f in ("src_class", "dst_class", "src_label", "dst_label", "direction", "layer", "proto", "is_ip")))
        assert np.array_equal(got, want)
        assert int(kc.metrics_group_hash(grouping, 0, 0)) == int(want[n])
    assert len(np.unique(nf.metrics_group_hash(0, g[:n]))) == n
    assert nf._lib.lib.nfagg_metrics_group_hash(0, None) == 0 == nf._lib.lib.nfagg_metrics_group_hash(nf._lib.MET_MAX_GROUPINGS, g.ctypes.data)     # bad arguments


def test_constants_are_read_from_the_source():
    m, pc = kc.metrics_constants(), kc.partition_constants()
    assert m["kMetLdsSlots"] & (m["kMetLdsSlots"] - 1) == 0 and 1 < m["kMetLdsProbe"] < m["kMetLdsSlots"] and m["kMetMinSlots"] >= m["kMetLdsSlots"]
    assert m["kMetFlowsPerBlock"] > 0
    assert pc["tile"] == pc["kPartBlock"] * pc["kPartRounds"] and pc["scan_chunk"] > 0 and pc["grid_cap"] > 0 and pc["kMaxShards"] >= 64
