"""The conversation fold (csrc/nfagg_conn.hip) where tests/test_conntrack_gpu.py does not reach: CRAFTED connection hashes under
contention, full tables, a table above 2^20 slots, the wave ballots' lane patterns and other clocks. The tuples come from
tests/golden/conntrack_crafted.json (searched by tests/conncraft.py; tests/test_conncraft_cpu.py derives them again):

    one_home     200 connections with one home slot of the 1 024-slot table, scattered: each 40 times, both directions, shuffled
                 among background connections over seven workgroups; far more than one probe round of eight
    wrap         40 connections on the last three slots of 1 024 (cap 512), 30 on the last three of 8 192 (cap 4 096), scattered
    same_word0   pairs of connections with one first key word and one home: per pair a whole wave A, B, A, B, ...; all the waves,
                 six workgroups of background, the waves again the other way round; both arrival orders
    full table   20 000 connections against caps 0, 1, 64 and 500 (1 024 slots each): TRUNCATED, `out` untouched, the hash ids
                 complete; a fitting call straight after it on the same handle; cap 0 over a stream with nothing tracked
    sized by n   cap 65 536 over 1 and over 3 000 flows: the table has 2 * min(cap, n) slots
    big table    1.2 M flows of 565 k connections, cap 600 000: 2^21 slots, so the scan of the block sums gives every lane two;
                 then a cap of exactly the count, and of one less (device entry point only)
    lanes        whole waves of 64 distinct connections with only lane 0 tracked, only lane 63, none, all, every other one and a
                 mix; a last wave of 1 and of 63 lanes; the cap is the connection count exactly
    times        five clocks around 1970 and the suite's; timestamps before, at and after mono_now, 0 and 2^64 - 1; the least
                 start and the greatest end in the first, a middle and the last flow; negative milliseconds
    no hash ids  hash_ids == NULL on both entry points

Expected values: the per-flow restatement (check_fold of tests/test_conntrack_gpu.py, through record_to_map and Python integers)
for everything up to some ten thousand flows, conncraft.fold above that. Everything is an integer and compared exactly, on the host
and the device entry point, with canaries over and behind `out` and the hash ids. A family's precondition is computed from the
partials the DEVICE returned (hash_total through conntrack_streams.home_slot) and printed."""
import ipaddress
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conncraft as cc  # noqa: E402
import conntrack_streams as ST  # noqa: E402
import test_conntrack_cpu as T  # noqa: E402
import test_conntrack_gpu as G  # noqa: E402
import test_netev_gpu as E  # noqa: E402
from test_conntrack_gpu import tab  # noqa: E402,F401  (fixture)

pytestmark = pytest.mark.gpu

CRAFTED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conntrack_crafted.json")))
FLOWS_PER_BLOCK = 1024                                                   # kConnFlowsPerBlock
CLOCKS = [0, -1, -5_000_000_001, 999_999_999, T.NOW]


def tuple_records(nf, tuples):
    a4 = lambda key: np.array([list(ipaddress.ip_address(t[key]).packed) for t in tuples], dtype=np.uint8)
    col = lambda key: np.array([t[key] for t in tuples])
    return cc.records(nf.FLOW_RECORD, a4("src"), col("sport"), a4("dst"), col("dport"), col("proto"))


def scattered(nf, tuples, rng, n_background, reps=40):
    """Every planted connection `reps` times, alternately in either direction, shuffled among flows of n_background background
    connections; at least seven workgroups long."""
    planted = np.repeat(tuple_records(nf, tuples), reps)
    planted = cc.turned(planted, np.arange(len(planted)) % 2 == 1)
    n = max(6 * FLOWS_PER_BLOCK + 777, len(planted) + 2000)
    pool = cc.distinct(nf.FLOW_RECORD, n_background)
    back = cc.both_ways(pool[rng.integers(0, n_background, n - len(planted))], rng)
    recs = cc.with_metrics(np.concatenate([planted, back])[rng.permutation(n)], rng)
    assert len(recs) >= 6 * FLOWS_PER_BLOCK + 777
    return recs


def homes(got, slots=1024):
    return np.array([ST.home_slot(int(h), slots) for h in got["hash_total"]])


def planted_both_ways(got, tuples, reps=40):
    mine = got[np.isin(got["hash_total"], np.array([int(t["total"], 16) for t in tuples], dtype=np.uint64))]
    assert len(mine) == len(tuples) and (mine["flows"] == reps // 2).all()


# ---- a. one home slot under contention
def test_two_hundred_connections_with_one_home_slot_scattered(nf, tab):
    tuples = CRAFTED["same_home"]
    got = G.check_fold(nf, tab, scattered(nf, tuples, np.random.default_rng(1), 200), cap=512)
    most = int(np.bincount(homes(got)).max())
    print("one_home: %d connections, %d share home slot %d of 1024 (precondition: >= 200)" % (len(got), most, int(np.bincount(homes(got)).argmax())))
    assert most >= 200 and len(got) <= 512
    planted_both_ways(got, tuples)


# ---- b. probe chains that wrap
@pytest.mark.parametrize("cap, family, n_background", [(512, "wrap_1024", 200), (4096, "wrap_8192", 2000)])
def test_probe_chains_that_wrap_the_end_of_the_table(nf, tab, cap, family, n_background):
    tuples = CRAFTED[family]
    recs = scattered(nf, tuples, np.random.default_rng(2), n_background)
    got = G.check_fold(nf, tab, recs, cap=cap)
    slots = 2 * cap
    n_last = int((homes(got, slots) >= slots - 3).sum())
    print("wrap: %d flows, %d connections, %d with a home in the last three of %d slots (precondition: >= %d)" % (len(recs), len(got), n_last, slots, len(tuples)))
    assert len(recs) > cap and n_last >= len(tuples) >= 30 and len(got) <= cap      # sized by the cap; ten connections per last slot
    planted_both_ways(got, tuples)


# ---- c. one first word, two second words, racing
@pytest.mark.parametrize("b_first", [False, True])
def test_pairs_with_one_first_key_word_racing(nf, tab, b_first):
    pairs = [(b, a) if b_first else (a, b) for a, b in CRAFTED["same_word0"]]
    waves = np.concatenate([tuple_records(nf, [pair[k % 2] for k in range(64)]) for pair in pairs])
    rng = np.random.default_rng(3)
    back = cc.both_ways(cc.distinct(nf.FLOW_RECORD, 300)[rng.integers(0, 300, 6 * FLOWS_PER_BLOCK)], rng)
    recs = cc.with_metrics(np.concatenate([waves, back, cc.turned(waves.copy(), np.ones(len(waves), dtype=bool))[::-1]]), rng)
    got = G.check_fold(nf, tab, recs, cap=512)
    key = (got["hash_total"] >> np.uint64(32)) * np.uint64(1024) + homes(got).astype(np.uint64)
    n_shared = int((np.unique(key, return_counts=True)[1] == 2).sum())
    print("same_word0: %d connections, %d pairs share the first key word and the home slot (precondition: >= %d >= 16)" % (len(got), n_shared, len(pairs)))
    assert n_shared >= len(pairs) >= 16 and len(got) <= 512
    mine = got[np.isin(got["hash_total"], np.array([int(t["total"], 16) for pair in pairs for t in pair], dtype=np.uint64))]
    assert len(mine) == 2 * len(pairs) and (mine["flows"] == 32).all()      # two connections per pair, each with its own sums


# ---- d. a full table
@pytest.fixture(scope="module")
def crowd(nf):
    """20 000 distinct connections, 500 discarded flows among them, and what the restatement makes of them."""
    rng = np.random.default_rng(4)
    recs = cc.distinct(nf.FLOW_RECORD, 20500, rng)
    recs["id"]["transport_protocol"][rng.choice(20500, 500, replace=False)] = 1
    parts, ids, n_disc = cc.fold(recs, T.NOW, T.MONO)
    assert (len(parts), n_disc) == (20000, 500)
    return recs, ids


@pytest.mark.parametrize("cap", [0, 1, 64, 500])
def test_a_table_that_fills_to_the_last_slot(nf, tab, crowd, cap):
    recs, ids = crowd
    rc, got, n_conns, got_ids, n_disc = G.fold_both(nf, tab, recs, cap=cap)      # fold_both: `out` untouched, both entry points above the cap
    assert rc == nf.TRUNCATED and len(got) == 0 and n_conns > cap and n_disc == 500
    assert np.array_equal(got_ids, ids)
    small = cc.seeded_stream(nf.FLOW_RECORD, 300, 40 + cap, 60)              # ... and nothing of it is left on the handle
    assert 50 < len(G.check_fold(nf, tab, small, cap=64)) <= 60


def test_cap_zero_over_a_stream_with_nothing_tracked(nf, tab):
    recs = cc.distinct(nf.FLOW_RECORD, 3000, np.random.default_rng(5))
    recs["id"]["transport_protocol"][::2] = 58
    recs["metrics"]["eth_protocol"][1::2] = 0x0806
    rc, got, n_conns, ids, n_disc = G.fold_both(nf, tab, recs, cap=0)
    assert (rc, len(got), n_conns, n_disc) == (nf.OK, 0, 0, 3000) and not ids.any()
    assert len(G.check_fold(nf, tab, recs, cap=0)) == 0


# ---- e. sized by the flows, not by the cap
@pytest.mark.parametrize("n", [1, 3000])
def test_a_large_cap_over_a_small_call(nf, tab, n):
    got = G.check_fold(nf, tab, cc.seeded_stream(nf.FLOW_RECORD, n, 6, 2000, discard_one_in=40), cap=65536)
    assert len(got) == 1 if n == 1 else 1000 < len(got) < 2000


# ---- the device entry point alone: f and i
def fold_device(nf, tab, d_recs, n, cap, now=T.NOW, mono=T.MONO, with_ids=True):
    """nfagg_conn_fold_device into a buffer of exactly the cap, with 0xAB canaries over it and behind it and the hash ids.
    Returns (rc, partials by first_idx, n_conns, hash ids or None, n_discarded)."""
    import torch
    d_ids = torch.full((n * 8 + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    d_out = torch.full((cap * 128 + 128,), 0xAB, dtype=torch.uint8, device="cuda")
    rc, n_conns, n_disc = tab.conn_fold_device(d_recs.data_ptr(), n, now, mono, d_ids.data_ptr() if with_ids else 0, cap, d_out.data_ptr())
    torch.cuda.synchronize()
    raw, raw_ids = d_out.cpu().numpy(), d_ids.cpu().numpy()
    used = n_conns * 128 if rc == nf.OK else 0
    assert (raw[used:] == 0xAB).all(), "bytes behind the partials were written"
    assert (raw_ids[n * 8 if with_ids else 0:] == 0xAB).all()
    return rc, G.by_first(raw[:used].copy().view(nf.CONN_PARTIAL)), n_conns, raw_ids[:n * 8].copy().view(np.uint64) if with_ids else None, n_disc


def assert_partials(got, want):
    assert len(got) == len(want)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 128) != want.view(np.uint8).reshape(-1, 128)).any(axis=1))
        raise AssertionError("%d of %d partials differ; the first, %d:\n got %r\nwant %r" % (len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))


def test_a_table_above_two_to_the_twenty_slots(nf, tab):
    n, cap = 1_200_000, 600_000
    recs = cc.seeded_stream(nf.FLOW_RECORD, n, 31, 690_000, discard_one_in=100)
    want, ids, n_disc = cc.fold(recs, T.NOW, T.MONO)
    slots = 1 << (2 * min(cap, n) - 1).bit_length()
    per = (slots // 1024 + 1023) // 1024
    print("big table: %d flows, %d connections, %d discarded; cap %d: %d slots, %d scan blocks, per = %d (preconditions: connections > 2^19, "
          "2 * min(cap, n) > 2^20)" % (n, len(want), n_disc, cap, slots, slots // 1024, per))
    assert 2 * min(cap, n) > 2**20 and 2**19 < len(want) <= cap and per == 2 and n_disc > 10000
    assert (want["flows"] > 0).all(axis=1).sum() > 100000 and (want["first_fin_idx"] != cc.NO_IDX).sum() > 100000
    d_recs = E.dev(recs)
    rc, got, n_conns, got_ids, got_disc = fold_device(nf, tab, d_recs, n, cap)
    assert (rc, n_conns, got_disc) == (nf.OK, len(want), n_disc)
    assert np.array_equal(got_ids, ids)
    assert_partials(got, want)
    rc, got, n_conns, _, _ = fold_device(nf, tab, d_recs, n, len(want))          # a cap of exactly the count: still 2^21 slots
    assert 2 * len(want) > 2**20 and (rc, n_conns) == (nf.OK, len(want))
    assert_partials(got, want)
    rc, got, n_conns, got_ids, got_disc = fold_device(nf, tab, d_recs, n, len(want) - 1)
    assert rc == nf.TRUNCATED and n_conns > len(want) - 1 and len(got) == 0 and got_disc == n_disc and np.array_equal(got_ids, ids)


# ---- g. lane patterns
PATTERNS = {"lane 0": lambda lane, wave: lane == 0, "lane 63": lambda lane, wave: lane == 63, "none": lambda lane, wave: lane < 0,
            "all": lambda lane, wave: lane >= 0, "alternating": lambda lane, wave: lane % 2 == 1,
            "mixed": lambda lane, wave: np.choose(wave % 6, [lane == 0, lane == 63, lane < 0, lane >= 0, lane % 2 == 0, lane < 32])}


@pytest.mark.parametrize("tail", [0, 1, 63])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_wave_ballots_on_lane_patterns_at_the_exact_cap(nf, tab, pattern, tail):
    n = 18 * 64 + tail                                                   # two workgroups; the last wave has `tail` lanes
    i = np.arange(n)
    keep = PATTERNS[pattern](i % 64, i // 64)
    recs = cc.distinct(nf.FLOW_RECORD, n, np.random.default_rng(7))             # every lane its own connection: every tracked lane wins
    recs["id"]["transport_protocol"][~keep & (i % 3 == 0)] = 1
    recs["metrics"]["eth_protocol"][~keep & (i % 3 != 0)] = 0x0806
    got = G.check_fold(nf, tab, recs, cap=int(keep.sum()))               # check_fold: n_discarded, partials and hash ids exactly
    assert len(got) == keep.sum() and got["first_idx"].tolist() == np.flatnonzero(keep).tolist()


# ---- h. times
@pytest.mark.parametrize("mono", [T.MONO, 7])
@pytest.mark.parametrize("now", CLOCKS)
def test_clocks_around_1970_and_timestamps_around_mono_now(nf, tab, now, mono):
    recs, where = cc.time_stream(nf.FLOW_RECORD, mono)
    got = G.check_fold(nf, tab, recs, cap=128, now=now, mono=mono)
    assert len(got) == len(where) == 72
    if now < 10**9:
        assert (got["start_ms_min"] < 0).sum() > 20 and (got["end_ms_max"] < 0).sum() >= 18
    else:
        assert (got["start_ms_min"] > 0).all()
    want, _, _ = cc.fold(recs, now, mono)                                # the second restatement agrees (it is (f)'s reference)
    assert_partials(got, want)


@pytest.mark.parametrize("n, now", [(513, -5_000_000_001), (513, 999_999_999), (4097, -5_000_000_001), (4097, 999_999_999)])
def test_the_seeded_records_under_other_clocks(nf, tab, n, now):
    recs = ST.seeded_records(nf, n, 12 + n)                              # ports around 128 / 256, unmapped addresses under 0x0800, times around MONO
    got = G.check_fold(nf, tab, recs, now=now)
    assert len(got) > n // 8 and (got["start_ms_min"] < 0).any() and (got["end_ms_max"] > 0).any()


# ---- i. no hash ids
def test_without_hash_ids_on_both_entry_points(nf, tab):
    recs = cc.seeded_stream(nf.FLOW_RECORD, 3000, 8, 700)
    want = G.check_fold(nf, tab, recs, cap=1024)
    rc, parts, n_conns, ids, n_disc = tab.conn_fold(recs, T.NOW, T.MONO, cap=1024, hash_ids=False)
    assert ids is None and (rc, n_conns) == (nf.OK, len(want)) and n_disc == int((~cc.tracked(recs)).sum())
    assert_partials(G.by_first(parts), want)
    rc, got, n_conns, ids, n_disc_d = fold_device(nf, tab, E.dev(recs), len(recs), 1024, with_ids=False)
    assert ids is None and (rc, n_conns, n_disc_d) == (nf.OK, len(want), n_disc)
    assert_partials(got, want)
