"""tests/keycraft.py itself, on the CPU: crafted keys hash to their targets under the helper's restatement, the library's host
function and the oracle's; the shard formula holds exactly on its boundaries; and the oracle — the reference that fold tests on
such streams compare with — keeps the flows of every family apart, in both modes."""
import numpy as np
import pytest

import keycraft as kc
from conftest import dedup_stream

M64 = (1 << 64) - 1
MASKS = ((1 << 16) - 1, (1 << 21) - 1)


def _three_hashes(nf, O, keys):
    mine = kc.key_hash(kc.as_words(keys))
    lib = np.array([nf.key_hash(k.tobytes()) for k in keys], dtype=np.uint64)
    orc = np.array([O.lib().orc_key_hash(np.ascontiguousarray(k).ctypes.data) for k in keys], dtype=np.uint64)
    return mine, lib, orc


def test_crafted_keys_hash_to_their_targets(nf, O):
    rng = np.random.default_rng(5)
    targets = np.array([0, 1, 2, 3, M64, M64 - 1, 1 << 63, 0x0123456789abcdef] * 1000, dtype=np.uint64)
    keys = kc.craft(targets, rng)                                    # 8000 DISTINCT keys (craft asserts it) over eight hashes
    assert keys.shape == (8000, 40) and not keys[:, 39].any()
    for got in _three_hashes(nf, O, keys[:800]):
        assert np.array_equal(got, targets[:800])
    # pinned words stay pinned; byte 39 is no part of the hash for the library and the oracle
    pinned = kc.craft(targets[:8], rng, fixed={0: 7, 4: np.arange(8)})
    w = kc.as_words(pinned)
    assert (w[:, 0] == 7).all() and np.array_equal(w[:, 4], np.arange(8, dtype=np.uint64))
    dirty = pinned.copy(); dirty[:, 39] = 0xa5
    _, lib, orc = _three_hashes(nf, O, dirty)
    assert np.array_equal(lib, targets[:8]) and np.array_equal(orc, targets[:8])


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name", [f for f in kc.FAMILIES if f != "one_bit"])
def test_family_targets_are_what_the_table_says(nf, O, name, mask):
    consts = kc.fold_constants()
    rng = np.random.default_rng(3)
    t = kc.family_targets(name, rng, mask, consts)
    keys = kc.craft(t, rng)
    for got in _three_hashes(nf, O, keys):
        assert np.array_equal(got, t)
    ti = [int(x) for x in t]
    win, ent = consts["window"], consts["kEntries"]
    if name == "same64":
        assert sorted(np.unique(t, return_counts=True)[1].tolist()) == sorted(kc.SAME64_GROUPS)
    elif name == "bit0":
        assert len(set(ti)) == 100 and all(a ^ 1 == b and a | 1 == b for a, b in zip(ti[::2], ti[1::2]))
    elif name.startswith("one_home"):
        assert len(set(ti)) == kc.ONE_HOME_K and len({x & ((1 << 21) - 1) for x in ti}) == 1
        assert ti[0] & mask == (mask if name == "one_home_ones" else mask - 5)
    elif name == "same_fp":
        assert len({x >> 18 for x in ti}) == 1 and len(ti) == 2 * win
        slots = [x & mask for x in ti]
        assert slots == list(range(slots[0], slots[0] + 2 * win))
        for parts in (256, consts["kSpillParts"]):                   # the border falls between the two middle slots for every partition count
            per = (mask + 1) // parts
            assert slots[win - 1] // per + 1 == slots[win] // per
    elif name == "cache_wrap":
        home = [(x >> 40) & (ent - 1) for x in ti]
        assert home.count(ent - 2) == home.count(ent - 1) == 2 * win
    elif name == "edge":
        assert set(ti) == {0, 1, 2, 3, 1 << 63, M64 - 1, M64}


@pytest.mark.parametrize("n_shards", [3, 4, 8])
def test_shard_of_on_the_boundaries_of_the_multiply_shift(nf, O, n_shards):
    rng = np.random.default_rng(n_shards)
    t = kc.shard_edge_targets(rng, n_shards)
    keys = kc.craft(t, rng)
    want = [((int(h) >> 32) * n_shards) >> 32 for h in t]
    assert sorted(set(want)) == list(range(n_shards))
    # both sides of every boundary are there: consecutive upper halves that land in different shards
    hi = sorted({int(h) >> 32 for h in t})
    assert sum(1 for a, b in zip(hi, hi[1:]) if b == a + 1 and (a * n_shards) >> 32 != (b * n_shards) >> 32) == n_shards - 1
    assert [nf.shard_of(k.tobytes(), n_shards) for k in keys] == want
    assert [O.lib().orc_shard_of(np.ascontiguousarray(k).ctypes.data, n_shards) for k in keys] == want
    recs = np.zeros(len(keys), dtype=O.FLOW_RECORD)                     # the host-side router of the sharded group takes records
    recs.view(np.uint8).reshape(len(recs), 144)[:, :40] = keys
    assert nf.distributed.shard_ids(recs, n_shards).tolist() == want


@pytest.fixture(scope="module")
def base_streams(O):
    th = O.zipf_thresholds(kc.N_FLOWS, 1.1)
    return {0: O.gen_stream(kc.N_RECORDS, seed=300, n_keys=kc.N_FLOWS, thresholds=th, variant=1),
            1: dedup_stream(O, kc.N_RECORDS, seed=301, n_keys=kc.N_FLOWS, thresholds=th, style=2)}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", kc.FAMILIES)
def test_the_oracle_keeps_crafted_flows_apart(O, base_streams, name, mode):
    """The number of evicted flows is the number of distinct keys, whatever their hashes: the oracle's map compares keys."""
    for mask in MASKS if name in ("one_home_m5", "same_fp") else MASKS[:1]:
        recs, keys, _ = kc.apply_family(base_streams[mode], name, mask)
        n = kc.distinct_flows(recs)
        assert n == kc.distinct_flows(base_streams[mode]) - (8 if name == "one_bit" else 0)
        want = O.run_accounter(recs, 1 << 20, mode)
        assert len(want) == 1 and len(want[0][1]) == n
        ev = np.ascontiguousarray(want[0][1]).view(np.uint8).reshape(n, 144)[:, :40]
        assert not ev[:, 39].any()
        evicted = {bytes(k) for k in ev}
        assert all(bytes(k) in evicted for k in keys)                # every planted flow comes out as itself
        # half of the planted flows are hot ones, half have a few records each
        # half of the planted flows took over the base stream's hottest ranks, half the ranks from COLD_RANK on: their record
        # counts are exactly the counts the base stream has at those ranks (remap changes keys, never which record is whose)
        col, k = len(keys) // 2, len(keys)
        base_inv, base_order = kc.flow_ranks(base_streams[mode])
        base_counts = np.bincount(base_inv)[base_order]
        flows, counts = np.unique(kc._key_column(recs), return_counts=True)
        planted = np.ascontiguousarray(keys).view(np.dtype((np.void, 40))).reshape(-1)
        got = np.sort(counts[np.searchsorted(flows, planted)])
        want_counts = np.sort(np.concatenate([base_counts[:col], base_counts[kc.COLD_RANK:kc.COLD_RANK + k - col]]))
        if name != "one_bit":
            assert np.array_equal(got, want_counts)
        assert base_counts[col - 1] > base_counts[kc.COLD_RANK] >= 1   # "hot" and "cold" are different things in this stream


def test_single_bit_neighbours_are_313_flows_and_byte_39_adds_none(O):
    rng = np.random.default_rng(9)
    nb = kc.one_bit_keys(rng)
    assert len(np.unique(nb, axis=0)) == 313 and not nb[:, 39].any()
    assert all(bin(int.from_bytes(bytes(a ^ nb[0]), "little")).count("1") == 1 for a in nb[1:])
    # These neighbours are not 313 hashes. Flipping bit b of key word i moves the value the step multiplies by +-2^b, hence the
    # hash state by +-2^b x kMul (mod 2^64). The next step rotates the state left by 27 and xors word i + 1 in, so a single-bit
    # flip of word i + 1 cancels the change exactly when the change is a single-bit flip of the state:
    #   b = 63: 2^63 x kMul = 2^63 (kMul is odd): the state's top bit, always. It lands on bit 26 of word i + 1.
    #   b = 62: 2^62 x kMul = 2^62 (kMul = 1 mod 4): bit 62 alone unless the addition carries into bit 63 — for half of all
    #           states. It lands on bit 25 of word i + 1.
    #   b < 62: 2^b x kMul has two or more bits set within the word (kMul = 5 mod 8): never a single-bit flip.
    # So of the neighbours of ANY key four pairs (words 0..3) share their hash for certain and up to four more may; nothing
    # else does. Flows one bit apart can share their 64-bit hash: the full-key compares are not only for adversaries.
    h = kc.key_hash(kc.as_words(nb))
    pairs = {(a, b) for a in range(1, 313) for b in range(a + 1, 313) if h[a] == h[b]}
    sure = {(1 + 64 * i + 63, 1 + 64 * (i + 1) + 26) for i in range(4)}
    maybe = {(1 + 64 * i + 62, 1 + 64 * (i + 1) + 25) for i in range(4)}
    assert sure <= pairs <= sure | maybe
    assert len(np.unique(h)) == 313 - len(pairs)
    recs = np.zeros(313 + 8, dtype=O.FLOW_RECORD)
    raw = recs.view(np.uint8).reshape(len(recs), 144)
    raw[:313, :40] = nb
    raw[313:, :40] = nb[0]
    raw[313:, 39] = 1 << np.arange(8)
    recs["metrics"]["packets"] = 1
    for mode in (0, 1):
        ev = O.run_accounter(recs[rng.permutation(len(recs))], 1 << 12, mode)[0][1]
        assert len(ev) == 313
        packets = {bytes(np.ascontiguousarray(e["id"]).view(np.uint8)[:39]): int(e["metrics"]["packets"]) for e in ev}
        assert packets[bytes(nb[0, :39])] == 9 and sorted(packets.values())[:312] == [1] * 312
