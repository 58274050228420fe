"""tests/basecraft.py on the CPU: the builder builds what it says (every sequence once, distinct keys, the position in the identity
fields), the oracle's Accounter on the families equals a restatement of model.AccumulateBase in plain Python integers — written
from pkg/model/flow_content.go:28-61 and pkg/flow/account.go:95, not from the oracle's C — in every layout, and the families have
TEETH: each of seventeen single-rule mutants of that restatement is told from the truth by scripts of the family that was built
for its rule."""
import json
import os

import numpy as np
import pytest

import basecraft as bc
import keycraft as kc

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "basecraft_digest.json")
SIZES = {"times": (7380, 28602), "lastnz": (7380, 28602), "macs": (16275, 48150), "sums": (4368, 12816), "wave": (64, 4096), "hot": (8, 32768)}
FOLDED = ("start", "end", "bytes", "packets", "flags", "eth_protocol", "src_mac", "dst_mac", "dscp", "sampling")
START, END, BYTES, PACKETS, FLAGS, ETH, SMAC, DMAC, DSCP, SAMPLING = range(10)

MUTANTS = {
    "times": ["start plain min", "start first non-zero", "start on low 32 bits", "end last non-zero", "end on low 32 bits"],
    "sums": ["bytes in 63 bits", "packets saturate"],
    "lastnz": ["eth first", "eth max", "dscp first", "dscp max", "sampling first", "sampling max"],
    "macs": ["mac last", "mac max", "zero by four bytes", "dst zero by two bytes"],
}


# ---------------------------------------------------------------- the restatement
def accumulate_base(p, o, mutant=None):
    """flow_content.go:28-61 on lists of Python integers (MACs: tuples of six bytes); p is changed in place. `mutant` swaps ONE
    rule for a plausible wrong one."""
    # time == 0 if the value has not been yet set
    if mutant == "start plain min":
        p[START] = min(p[START], o[START])
    elif mutant == "start first non-zero":
        if p[START] == 0:
            p[START] = o[START]
    elif mutant == "start on low 32 bits":
        if p[START] == 0 or ((p[START] & M32) > (o[START] & M32) and o[START] != 0):
            p[START] = o[START]
    elif p[START] == 0 or (p[START] > o[START] and o[START] != 0):
        p[START] = o[START]
    if mutant == "end last non-zero":
        if o[END] != 0:
            p[END] = o[END]
    elif mutant == "end on low 32 bits":
        if p[END] == 0 or (p[END] & M32) < (o[END] & M32):
            p[END] = o[END]
    elif p[END] == 0 or p[END] < o[END]:
        p[END] = o[END]
    p[BYTES] = (p[BYTES] + o[BYTES]) & (M64 >> 1 if mutant == "bytes in 63 bits" else M64)            # uint64 +=
    p[PACKETS] = min(p[PACKETS] + o[PACKETS], M32) if mutant == "packets saturate" else (p[PACKETS] + o[PACKETS]) & M32   # uint32 +=
    p[FLAGS] |= o[FLAGS]
    for f, what in ((ETH, "eth"), (DSCP, "dscp"), (SAMPLING, "sampling")):
        if mutant == what + " first":
            if p[f] == 0:
                p[f] = o[f]
        elif mutant == what + " max":
            p[f] = max(p[f], o[f])
        elif o[f] != 0:
            p[f] = o[f]
    for f in (SMAC, DMAC):
        if mutant == "mac last":
            if any(o[f]):
                p[f] = o[f]
        elif mutant == "mac max":
            p[f] = max(p[f], o[f])
        elif mutant == "zero by four bytes":
            if not any(p[f][:4]):
                p[f] = o[f]
        elif mutant == "dst zero by two bytes" and f == DMAC:
            if not any(p[f][:2]):
                p[f] = o[f]
        elif not any(p[f]):                                          # AllZerosMac
            p[f] = o[f]


def columns(fam):
    """The ten folded fields of every record as Python integers (MACs as tuples), record by record."""
    m = fam.recs["metrics"]
    cols = [m[f].tolist() for f in FOLDED]
    cols[SMAC], cols[DMAC] = [tuple(x) for x in cols[SMAC]], [tuple(x) for x in cols[DMAC]]
    return list(zip(*cols))


def fold_scripts(fam, rows, mutant=None):
    """One Accounter entry per script: the first record stored whole (account.go:95), the others accumulated in the script's order.
    Returns the ten folded fields per script."""
    out = []
    for a, n in zip(fam.start.tolist(), fam.length.tolist()):
        p = list(rows[a])
        for o in rows[a + 1:a + n]:
            accumulate_base(p, o, mutant)
        out.append(tuple(p))
    return out


def as_records(fam, folded):
    """The flows the restatement leaves, as records: every script's FIRST record with the ten folded fields replaced."""
    out = fam.recs[fam.start].copy()
    m = out["metrics"]
    for f, name in enumerate(FOLDED):
        m[name] = np.array([row[f] for row in folded], dtype=np.uint8 if name.endswith("_mac") else np.uint64)
    return out


@pytest.fixture(scope="module")
def truth():
    cache = {}

    def get(name):
        if name not in cache:
            fam = bc.family(name)
            rows = columns(fam)
            cache[name] = (fam, rows, fold_scripts(fam, rows))
        return cache[name]
    return get


# ---------------------------------------------------------------- the builder
@pytest.mark.parametrize("name", bc.FAMILIES)
def test_families_have_the_sizes_the_issue_names_and_one_key_per_script(name):
    fam = bc.family(name)
    assert (fam.n_scripts, len(fam.recs)) == SIZES[name] and len(fam.recs) < bc.MAX_RECORDS
    assert kc.distinct_flows(fam.recs) == fam.n_scripts == len(np.unique(fam.keys, axis=0))
    raw = fam.recs.view(np.uint8).reshape(-1, 144)
    assert not raw[:, 39].any() and np.array_equal(raw[:, :39], fam.keys[fam.script, :39])
    m = fam.recs["metrics"]
    assert np.array_equal(m["if_index_first_seen"], 1 + fam.pos) and np.array_equal(m["direction_first_seen"], fam.pos & 1)
    assert np.array_equal(m["ssl_version"], 0x0300 + fam.pos)
    assert not (m["start"] == M64).any()                                 # the one value the slots cannot hold (include/nfagg.h)
    assert bc.family(name) is fam                                        # built once


@pytest.mark.parametrize("name", bc.EXHAUSTIVE)
def test_exhaustive_families_hold_every_sequence_once(name):
    fam = bc.family(name)
    n_sym, max_len = bc.N_SYMBOLS[name], bc.MAX_LEN[name]
    assert fam.n_scripts == sum(n_sym ** k for k in range(1, max_len + 1))
    assert len(fam.recs) == sum(k * n_sym ** k for k in range(1, max_len + 1))
    sym = fam.symbol_numbers()                                           # from the records' bytes
    strings = {tuple(sym[a:a + n]) for a, n in zip(fam.start, fam.length)}
    assert len(strings) == fam.n_scripts and {len(s) for s in strings} == set(range(1, max_len + 1))
    assert set(sym.tolist()) == set(range(n_sym))
    assert sum(k * n_sym ** k for k in range(1, max_len + 2)) >= bc.MAX_RECORDS      # one length more would pass the limit
    assert fam.describe(0).endswith("'0'")


def test_symbols_by_their_fields():
    """The symbol of every record once more, from the VALUES the issue's table lists (not through the builder's setters)."""
    fam = bc.family("times")
    m, sym = fam.recs["metrics"], fam.symbol_numbers()
    cls = {0: 0, (1 << 32) + 5: 1, 7: 2}
    assert [3 * cls[s] + cls[e] for s, e in zip(m["start"].tolist(), m["end"].tolist())] == sym.tolist()
    fam = bc.family("lastnz")
    m, sym, t = fam.recs["metrics"], fam.symbol_numbers(), fam.pos
    d = np.where(m["dscp"] == 0, 0, np.where(m["dscp"] == 40 + t, 1, 2))
    s = np.where(m["sampling"] == 0, 0, np.where(m["sampling"] == 1 + t, 1, 2))
    e = np.where(m["eth_protocol"] == 0, 0, np.where(m["eth_protocol"] == 0x0800 + t, 1, 2))
    assert np.array_equal(3 * d + s, sym) and np.array_equal(e, (d + s) % 3)
    assert (m["dscp"][d == 2] == 0xFF - t[d == 2]).all() and (m["sampling"][s == 2] == 0xFFFFFFFF - t[s == 2]).all()
    assert (m["eth_protocol"][e == 2] == 0xFFFF - t[e == 2]).all() and (m["sampling"] == 0xFFFFFFFF).any() and (m["eth_protocol"] == 0xFFFF).any()
    fam = bc.family("macs")
    m, sym = fam.recs["metrics"], fam.symbol_numbers()

    def shape(mac):
        lo32, hi16 = mac[:, :4].any(axis=1), mac[:, 4:].any(axis=1)
        return np.where(~lo32 & ~hi16, 0, np.where(lo32 & ~hi16, 1, np.where(~lo32 & hi16, 3, np.where(mac[:, 0] == 0, 2, 4))))
    assert np.array_equal(5 * shape(m["src_mac"]) + shape(m["dst_mac"]), sym)
    assert not m["sampling"].any() and not m["dscp"].any()
    fam = bc.family("sums")
    m, sym = fam.recs["metrics"], fam.symbol_numbers()
    b, p = {v: k for k, v in enumerate(bc.BYTES)}, {v: k for k, v in enumerate(bc.PACKETS)}
    assert [4 * b[x] + p[y] for x, y in zip(m["bytes"].tolist(), m["packets"].tolist())] == sym.tolist()
    assert np.array_equal(m["flags"], 1 << ((3 * fam.pos + sym) % 16))


@pytest.mark.parametrize("name", ["lastnz", "macs"])
def test_no_two_records_of_a_script_agree_in_a_non_zero_field(name):
    fam = bc.family(name)
    m = fam.recs["metrics"]
    for f in ("dscp", "sampling", "eth_protocol") if name == "lastnz" else ("src_mac", "dst_mac"):
        v = m[f].astype(np.uint64)
        if v.ndim == 2:
            v = (v << (8 * np.arange(6, dtype=np.uint64))).sum(axis=1)
        nz = v != 0
        pairs = np.stack([fam.script[nz].astype(np.uint64), v[nz]], axis=1)
        assert len(np.unique(pairs, axis=0)) == nz.sum(), f
    if name == "macs":
        s, d = m["src_mac"], m["dst_mac"]
        assert not ((s == d).all(axis=1) & s.any(axis=1)).any()            # dst is offset from src


def test_seeded_families_have_the_asked_shapes():
    wave, hot = bc.family("wave"), bc.family("hot")
    assert (wave.length == 64).all() and (wave.start % 64 == 0).all() and (hot.length == 4096).all()
    for fam in (wave, hot):
        sym = fam.symbol_numbers()
        assert fam.n_symbols == len(bc.UNION) == 59 and set(sym.tolist()) == set(range(59))
    m = hot.recs["metrics"]
    for s in range(hot.n_scripts):                                       # neither end nor start is monotone along a hot script
        r = hot.records_of(s)["metrics"]
        assert (np.diff(r["end"].astype(np.int64)) < 0).sum() > 100 and (np.diff(r["start"].astype(np.int64)) < 0).sum() > 100
    assert (m["end"] == bc.END_A).any() and (m["start"] == bc.END_B).any()


def test_digests_are_the_pinned_ones():
    with open(GOLDEN) as f:
        pinned = json.load(f)
    assert {name: bc.digest(bc.family(name)) for name in bc.FAMILIES} == pinned


# ---------------------------------------------------------------- the oracle equals the restatement
@pytest.mark.parametrize("name", bc.FAMILIES)
def test_oracle_equals_the_python_restatement_in_every_layout(O, truth, name):
    fam, _, folded = truth(name)
    want = as_records(fam, folded)
    rm, _ = bc.round_major(fam)
    for layout, order in (("flow_major", bc.flow_major(fam)), ("round_major", rm), ("shuffled", bc.shuffled(fam))):
        ev = O.run_accounter(fam.recs[order], 1 << 20, 0)
        assert len(ev) == 1 and len(ev[0][1]) == fam.n_scripts
        got = ev[0][1]
        got = got[np.argsort(fam.scripts_of(got))]                       # script order
        g, w = got.view(np.uint8).reshape(-1, 144), want.view(np.uint8).reshape(-1, 144)
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert len(bad) == 0, "%s, %s: %d scripts differ, first %s" % (name, layout, len(bad), fam.describe(int(bad[0])))


# ---------------------------------------------------------------- the families have teeth
@pytest.mark.parametrize("name", list(MUTANTS))
def test_every_mutant_is_told_apart_by_its_family(truth, name):
    fam, rows, folded = truth(name)
    print()
    for mutant in MUTANTS[name]:
        wrong = fold_scripts(fam, rows, mutant)
        differ = [s for s, (a, b) in enumerate(zip(wrong, folded)) if a != b]
        print("%-7s %-24s told apart by %5d of %5d scripts%s" % (name, mutant, len(differ), fam.n_scripts, ", first " + fam.describe(differ[0]) if differ else ""))
        assert differ, "%s: no script of %s tells it from the truth" % (mutant, name)
