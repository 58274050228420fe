"""Streams whose ADDRESSES have chosen sketch hashes (a helper module, no fixtures). keycraft.craft_ip builds an address for any
ip_hash value; here families of such addresses are planted into a seeded stream, so that the HyperLogLog registers and the
Count-Min counters see what 30 000 random addresses never give them:

    rho_ladder   the four registers of word 0, the four of the last word and eight random ones; one address for every rho from 1
                 to 64 - p + 1 per register; in arrival order rho rises for half of the registers (every address raises its
                 register) and falls for the other half (the first address sets the maximum, the others must leave it alone)
    sentinel     all remainder bits zero in registers 0 and m - 1 (rho = 64 - p + 1: only the sentinel bit ends the count), and
                 the hashes 0 and 2^64 - 1
    one_word     the four registers of ONE 32-bit word, 64 addresses each with rising rho; a block of 256 records at the head of
                 the stream holds them interleaved, so that every wave of 64 records raises all four registers through the
                 compare-and-swap on their common word
    half_half    p = 18 only, a stream of its own: 2^17 addresses with rho = 1 in the lower half of the registers, 2^17 with
                 rho = 47 in the upper half (the registers on which a HyperLogLog sum added up in doubles goes wrong)
    cm_first / cm_last   300 addresses each on counter 0 / counter 2^log2w - 1 of Count-Min row 0 (seed index 0 picks row 0's
                 counter; the other rows fall where they fall), byte counts 0, 1, 2^32 - 1, 2^32, 2^63, 2^64 - 1 on their records

The src addresses carry rho_ladder and cm_first, the dst addresses sentinel, one_word and cm_last: half of each family on the
stream's hottest flows, half on cold ones."""
import zlib

import numpy as np

import keycraft as kc

_u = np.uint64
HLL_SEED, CM_SEED = 2, 0
N_RECORDS, N_FLOWS, COLD_RANK = 150_000, 5_000, 2_500
CM_FAMILY = 300
EDGE_BYTES = np.array([0, 1, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1], dtype=np.uint64)
# (hll_p, cm_depth, cm_log2_width): the limits of the configuration (nfagg_create: p 4..18, depth 1..8, log2 width from 4)
CONFIGS = [(4, 1, 4), (10, 8, 4), (18, 8, 16)]


def max_rho(p):
    return 64 - p + 1


def hll_targets(p, regs, rhos, rng):
    """One ip_hash(., 2) value per (register, rho): the register's index in the top p bits, then rho - 1 zeroes, a one and random
    bits below it — or nothing but zeroes for rho = 64 - p + 1."""
    regs, rhos = np.asarray(regs, dtype=np.uint64), np.asarray(rhos, dtype=np.int64)
    assert ((1 <= rhos) & (rhos <= max_rho(p))).all() and (regs < (1 << p)).all()
    rem_bits = 64 - p
    rem = np.zeros(len(regs), dtype=np.uint64)
    some = rhos <= rem_bits
    below = (rem_bits - rhos[some]).astype(np.uint64)                                    # random bits below the leading one
    rem[some] = (_u(1) << below) | (rng.integers(0, 1 << 62, size=int(some.sum()), dtype=np.uint64) & ((_u(1) << below) - _u(1)))
    return (regs << _u(rem_bits)) | rem


def rho_of(h, p):
    """(register, rho) of ip_hash values, in Python integers."""
    out = []
    for x in np.asarray(h, dtype=np.uint64).tolist():
        w = ((x << p) & kc.M64) | (1 << (p - 1))
        out.append((x >> (64 - p), 64 - w.bit_length() + 1))
    return out


def ladder_registers(p, rng):
    m = 1 << p
    edge = [0, 1, 2, 3, m - 4, m - 3, m - 2, m - 1]
    if m == 16:                                                                           # p = 4: word 0, the last word and the two between are all there is
        return np.arange(16)
    return np.concatenate([edge, rng.permutation(m - 8)[:8] + 4])


def rho_ladder(p, rng):
    """Addresses in the arrival order wanted: step by step through the ladder, every register once per step; rho rises with the
    steps for the even positions of ladder_registers and falls for the odd ones."""
    regs, top = ladder_registers(p, rng), max_rho(p)
    reg_col, rho_col = [], []
    for step in range(top):
        for k, r in enumerate(regs):
            reg_col.append(r)
            rho_col.append(step + 1 if k % 2 == 0 else top - step)
    return kc.craft_ip(hll_targets(p, reg_col, rho_col, rng), HLL_SEED, rng)


def sentinel(p, rng, copies=4):
    m = 1 << p
    t = [0, (m - 1) << (64 - p), kc.M64] * copies                                        # hash 0 IS register 0's sentinel case
    return kc.craft_ip(np.array(t, dtype=np.uint64), HLL_SEED, rng)


def one_word(p, rng):
    """(256, 16) addresses in BLOCK order: record k of the block is register 4 w + k % 4 with the (k // 4)-th rho of 64 rising
    ones (1 .. 64 - p + 1, each value once or twice)."""
    m, top = 1 << p, max_rho(p)
    word = int(rng.integers(1, m // 4 - 1)) if m > 16 else 1
    k = np.arange(256)
    return kc.craft_ip(hll_targets(p, 4 * word + k % 4, 1 + (k // 4) * top // 64, rng), HLL_SEED, rng), word


def cm_family(log2w, last, rng, n=CM_FAMILY):
    low = rng.integers(0, 1 << (64 - log2w), size=n, dtype=np.uint64)
    top = _u(((1 << log2w) - 1) << (64 - log2w)) if last else _u(0)
    return kc.craft_ip(top | low, CM_SEED, rng)


def hot_and_cold(k, rng, skip=0):
    """kc.hot_and_cold_ranks for this module's stream: half on the hottest ranks, half from COLD_RANK on, dealt at random.
    skip: leave out the first `skip` ranks of either half (the ranks another hot_and_cold(2 * skip) took)."""
    assert skip + k // 2 <= COLD_RANK and COLD_RANK + skip + k - k // 2 <= N_FLOWS - 500
    ranks = np.concatenate([skip + np.arange(k // 2), COLD_RANK + skip + np.arange(k - k // 2)])
    return ranks[rng.permutation(k)]


def plant(base, plan):
    """A copy of `base` in which, for every (side, ranks, addresses, by_arrival) of the plan, the flow of rank ranks[k] carries
    addresses[k] as its src (side 0) or dst (side 1) address in all its records. by_arrival: the addresses go to the chosen flows
    in the order of the flows' first records instead. Ranks are those of `base` (one plan = one look at the base stream).
    Returns (records, [record mask of each plan entry])."""
    inverse, order = kc.flow_ranks(base)
    n_flows = len(order)
    first = np.full(n_flows, len(base), dtype=np.int64)
    np.minimum.at(first, inverse, np.arange(len(base)))
    out = np.ascontiguousarray(base).copy()
    raw = out.view(np.uint8).reshape(len(out), 144)
    masks, used = [], {0: set(), 1: set()}
    for side, ranks, addrs, by_arrival in plan:
        ranks = np.asarray(ranks).reshape(-1)
        assert len(ranks) == len(addrs) and ranks.max() < n_flows, "the stream has only %d flows" % n_flows
        assert not (used[side] & set(ranks.tolist())) and len(set(ranks.tolist())) == len(ranks)
        used[side] |= set(ranks.tolist())
        flows = order[ranks]
        if by_arrival:
            flows = flows[np.argsort(first[flows], kind="stable")]
        new = np.full(n_flows, -1, dtype=np.int64)
        new[flows] = np.arange(len(addrs))
        k = new[inverse]
        hit = k >= 0
        raw[hit, 16 * side:16 * side + 16] = addrs[k[hit]]
        masks.append(hit)
    return out, masks


def planted_stream(O, p, depth, log2w):
    """The base stream (variant 1: bytes wrap) with every family of the configuration planted. Returns (records, info): info has
    the planted addresses per family, the block's word, and the number of distinct flows."""
    rng = np.random.default_rng(zlib.crc32(b"sketchcraft") + 1000 * p + 10 * depth + log2w)
    th = O.zipf_thresholds(N_FLOWS, 1.1)
    base = O.gen_stream(N_RECORDS, seed=400, n_keys=N_FLOWS, thresholds=th, variant=1)
    lad, cm0 = rho_ladder(p, rng), cm_family(log2w, False, rng)
    sen, (blk, word), cm1 = sentinel(p, rng), one_word(p, rng), cm_family(log2w, True, rng)
    src_ranks, dst_ranks = hot_and_cold(len(lad) + len(cm0), rng), hot_and_cold(len(sen) + len(cm1), rng)
    # the block's flows keep the src address they have: their records come first in the stream, and a ladder address among them
    # would arrive before its step of the ladder
    blk_ranks = hot_and_cold(len(blk), rng, skip=(len(src_ranks) + 1) // 2)
    assert not set(blk_ranks.tolist()) & (set(src_ranks.tolist()) | set(dst_ranks.tolist()))
    lad_ranks = np.sort(src_ranks[:len(lad)])                                            # by_arrival deals them; hot and cold alike
    plan = [(0, lad_ranks, lad, True), (0, src_ranks[len(lad):], cm0, False),
            (1, dst_ranks[:len(sen)], sen, False), (1, blk_ranks, blk, False), (1, dst_ranks[len(sen):], cm1, False)]
    recs, masks = plant(base, plan)
    assert kc.distinct_flows(recs) == kc.distinct_flows(base), "planting must not merge or split flows"
    for hit in (masks[1], masks[4]):                                                     # the byte edges, record by record, on both counter families
        at = np.flatnonzero(hit)
        recs["metrics"]["bytes"][at] = EDGE_BYTES[np.arange(len(at)) % len(EDGE_BYTES)]
    # the block: one record of each one_word flow, in block order, at the head of the stream (copies of records of flows the
    # stream holds already: the flows stay what they are, their first record changes)
    raw = recs.view(np.uint8).reshape(len(recs), 144)
    dst_col = np.ascontiguousarray(raw[:, 16:32]).view(np.dtype((np.void, 16))).reshape(-1)
    pos = {bytes(a): None for a in blk}
    for i in np.flatnonzero(masks[3]):
        if pos[bytes(dst_col[i])] is None:
            pos[bytes(dst_col[i])] = i
    head = recs[[pos[bytes(a)] for a in blk]]
    recs = np.concatenate([head, recs])
    assert kc.distinct_flows(recs) == kc.distinct_flows(base)
    return recs, dict(rho_ladder=lad, sentinel=sen, one_word=blk, word=word, cm_first=cm0, cm_last=cm1, flows=kc.distinct_flows(base))


_PLANTED = {}


def planted_streams(O):
    """{p: (records, info, the oracle's (cm_src, cm_dst, hll_src, hll_dst))} for every configuration of CONFIGS, built once per
    process and shared by the CPU and the GPU tests; nobody writes to it."""
    if not _PLANTED:
        for p, depth, log2w in CONFIGS:
            recs, info = planted_stream(O, p, depth, log2w)
            _PLANTED[p] = (recs, info, O.sketches(recs, depth, log2w, p))
    return _PLANTED


def seeded_registers():
    """(p, n, registers) with geometric register values, as a real HyperLogLog holds them for about n items: the inputs of the
    estimator tests (tests/test_host_logic.py, tests/test_crafted_sketches_cpu.py)."""
    rng = np.random.default_rng(11)
    for p, n in ((14, 50), (14, 20000), (14, 400000), (10, 3000), (4, 3), (16, 5_000_000)):
        regs = np.zeros(1 << p, dtype=np.uint8)
        idx = rng.integers(0, 1 << p, size=min(n, 2_000_000))
        rho = np.minimum(rng.geometric(0.5, size=idx.size), 64 - p + 1).astype(np.uint8)
        np.maximum.at(regs, idx, rho)
        yield p, n, regs


def half_half_stream(O):
    """2^18 records, one flow each: record i's src address is the i-th of 2^17 addresses with rho = 1 in registers 0 .. 2^17 - 1
    followed by 2^17 with rho = 47 in registers 2^17 .. 2^18 - 1 (p = 18), shuffled."""
    p, half = 18, 1 << 17
    rng = np.random.default_rng(zlib.crc32(b"half_half"))
    regs = np.arange(2 * half)
    addrs = kc.craft_ip(hll_targets(p, regs, np.where(regs < half, 1, max_rho(p)), rng), HLL_SEED, rng)
    recs = O.gen_stream(2 * half, seed=401, n_keys=N_FLOWS, thresholds=O.zipf_thresholds(N_FLOWS, 1.1), variant=1)
    recs.view(np.uint8).reshape(len(recs), 144)[:, :16] = addrs[rng.permutation(2 * half)]
    return recs


def half_half_registers():
    regs = np.ones(1 << 18, dtype=np.uint8)
    regs[1 << 17:] = max_rho(18)
    return regs


def check_preconditions(O, p, log2w, sk, info):
    """On the ORACLE's arrays (cm_src, cm_dst, hll_src, hll_dst) of a planted stream: every family reached its branch. A register
    keeps its maximum only, so "every rho occurs" is asked of the oracle's update address by address, each into an empty array."""
    import ctypes as C
    cm_s, cm_d, hs, hd = sk
    m, top = 1 << p, max_rho(p)
    for name, regs in (("src", hs), ("dst", hd)):
        assert int(regs.max()) == top, "%s: the largest register is %d, not %d" % (name, regs.max(), top)
        assert regs[0] != 0 and regs[m - 1] != 0, name
    seen = {}
    for a in info["rho_ladder"]:
        one = np.zeros(m, dtype=np.uint8)
        O.lib().orc_hll_update(one.ctypes.data_as(C.c_void_p), p, a.tobytes())
        reg = int(np.flatnonzero(one)[0])
        seen.setdefault(reg, set()).add(int(one[reg]))
    assert len(seen) == 16 and all(v == set(range(1, top + 1)) for v in seen.values()), "every rho value occurs, in each of 16 registers"
    assert {0, 1, 2, 3, m - 4, m - 3, m - 2, m - 1} <= set(seen) and all(hs[r] == top for r in seen)
    assert hd[0] == top and hd[m - 1] == top, "the sentinel cases of registers 0 and m - 1"
    assert cm_s[0] != 0 and cm_d[(1 << log2w) - 1] != 0, "row 0's first (src) and last (dst) counter"


def exact_hll_estimate(regs, p):
    """The HyperLogLog estimate in exact arithmetic, rounded once. Returns (estimate, distance of the raw estimate from the
    branch point 2.5 m in ULPs of 2.5 m, as a float; inf when there is no zero register and no branch)."""
    import math
    from fractions import Fraction
    hist = np.bincount(np.asarray(regs, dtype=np.uint8), minlength=65)
    m = 1 << p
    alpha = 0.673 if p == 4 else 0.697 if p == 5 else 0.709 if p == 6 else 0.7213 / (1.0 + 1.079 / float(m))
    total = sum(int(hist[k]) << (64 - k) for k in range(65))                              # 2^64 * sum of 2^-reg
    raw = Fraction(alpha) * m * m * (1 << 64) / total
    zeros = int(hist[0])
    if not zeros:
        return float(raw), math.inf
    edge = 2.5 * m
    gap = float(abs(raw - Fraction(edge)) / Fraction(np.spacing(edge)))
    return (float(m) * math.log(float(m) / float(zeros)) if raw <= Fraction(edge) else float(raw)), gap


def ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b))) if a != b else 0.0
