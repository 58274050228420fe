"""tests/conncraft.py, the conversation fold over arrays, held against what it restates: its hashes against the per-flow
restatement (tests/conntrack_ref.py) and the library's host-side nfagg_conn_hash on random tuples of every message class; its fold
against conntrack_ref.fold on vector records, on a seeded stream of the fixed-length class (discarded flows, both directions, FIN,
flags on UDP and SCTP) and on the time cases under five clocks; and every family of tests/golden/conntrack_crafted.json derived
again from conntrack_streams.home_slot and the per-flow restatement."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conncraft as cc  # noqa: E402
import conntrack_ref as CT  # noqa: E402
import conntrack_streams as ST  # noqa: E402
import test_conntrack_cpu as T  # noqa: E402

CRAFTED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conntrack_crafted.json")))
CLOCKS = [0, -1, -5_000_000_001, 999_999_999, T.NOW]


def text4(a):
    return b"%d.%d.%d.%d" % tuple(int(x) for x in a)


def random_tuples(rng, n):
    edge = np.array([100, 101, 109, 110, 199, 200, 254, 255])
    src4, dst4 = (np.concatenate([np.full((n, 1), 10), np.where(rng.integers(0, 3, (n, 3)) > 0, rng.integers(100, 256, (n, 3)), rng.choice(edge, (n, 3)))], axis=1)
                  for _ in range(2))
    ports = np.array([1024, 1025, 1279, 1280, 32767, 32768, 65280, 65535])
    sport, dport = (np.where(rng.integers(0, 3, n) > 0, rng.integers(1024, 65536, n), rng.choice(ports, n)) for _ in range(2))
    return src4.astype(np.uint8), sport, dst4.astype(np.uint8), dport


def test_the_partial_layout_is_the_products(nf):
    assert cc.CONN_PARTIAL == nf.CONN_PARTIAL and cc.NO_IDX == nf._lib.CONN_NO_IDX


@pytest.mark.parametrize("proto", [6, 17, 132])
def test_hashes_against_the_per_flow_restatement_and_the_library(nf, proto):
    rng = np.random.default_rng(proto)
    n = 300
    src4, sport, dst4, dport = random_tuples(rng, n)
    src4[:3], dst4[:3] = [[10, 100, 100, 100], [10, 255, 255, 255], [10, 200, 100, 255]], [[10, 255, 255, 255], [10, 100, 100, 100], [10, 200, 100, 255]]
    sport[2] = dport[2] = 4000                                           # src == dst: hashA == hashB
    a, b = cc.side_hash(src4, sport), cc.side_hash(dst4, dport)
    t = cc.totals(a, b, proto)
    recs = cc.records(nf.FLOW_RECORD, src4, sport, dst4, dport, proto)
    assert np.array_equal(cc.side_hash(recs["id"]["src_ip"], sport), a)   # the record's sixteen bytes are taken too
    for i in range(n):
        fl = {b"SrcAddr": text4(src4[i]), b"SrcPort": int(sport[i]), b"DstAddr": text4(dst4[i]), b"DstPort": int(dport[i]), b"Proto": proto}
        want = CT.compute_hash(fl, T.KD)
        assert (int(a[i]), int(b[i]), int(t[i])) == want
        assert nf.conn_hash(recs[i].tobytes()) == (want[2], want[0], want[1])
        assert want == cc.plain_hashes(fl[b"SrcAddr"].decode(), fl[b"SrcPort"], fl[b"DstAddr"].decode(), fl[b"DstPort"], proto)
    assert a[2] == b[2] and len(np.unique(t)) == n


def test_the_hash_of_one_fixed_address():
    ports = np.array([1024, 2047, 3071, 65535])
    for addr in (cc.GOLDEN_SRC, cc.GOLDEN_DST, "2001:db8::1"):
        got = cc.fixed_side_hash(addr, ports)
        assert got.tolist() == [CT.fnv64a(CT.to_bytes(int(p)), CT.fnv64a(CT.to_bytes(addr.encode()))) for p in ports]


def test_what_the_restatement_refuses():
    ok4 = np.array([[10, 100, 100, 100]], dtype=np.uint8)
    for bad4, port in (([[10, 99, 100, 100]], 2000), ([[11, 100, 100, 100]], 2000), ([[10, 100, 100, 100]], 1023)):
        with pytest.raises(AssertionError):
            cc.side_hash(np.array(bad4, dtype=np.uint8), np.array([port]))
    with pytest.raises(AssertionError):
        cc.totals(cc.side_hash(ok4, np.array([2000])), cc.side_hash(ok4, np.array([2001])), 1)


def assert_folds_agree(nf, recs, now=T.NOW, mono=T.MONO):
    parts, ids, n_disc = CT.fold(T.maps(recs, now, mono), T.KD)
    got, got_ids, got_disc = cc.fold(recs, now, mono)
    assert (got_ids.tolist(), got_disc) == (ids, n_disc)
    want = T.partial_array(nf, parts)
    if got.tobytes() != want.tobytes():
        k = next(i for i in range(min(len(want), len(got))) if got[i].tobytes() != want[i].tobytes())
        raise AssertionError("partial %d of %d / %d:\n got %r\nwant %r" % (k, len(got), len(want), got[k], want[k]))
    return got


def test_fold_on_vector_records(nf):
    a, b, c = ("10.100.100.100", 40000), ("10.100.100.101", 4443), ("10.255.255.255", 65535)
    fl = lambda s, d, **kw: dict(src=s[0], sport=s[1], dst=d[0], dport=d[1], **{**dict(proto=6, bytes=100, packets=2, flags=0x10), **kw})
    flows = [fl(a, b), fl(b, a, bytes=7), fl(c, c, proto=17, flags=0x11), fl(a, b, proto=1), fl(a, c, proto=132, bytes=0, packets=0),
             fl(b, a, flags=0x11), fl(a, b, flags=0x01), fl(c, c, proto=17), fl(c, a, proto=132, bytes=(1 << 64) - 1), fl(a, c, proto=132, bytes=5)]
    got = assert_folds_agree(nf, T.records(nf, flows))
    assert got["flows"].tolist() == [[2, 2], [2, 0], [2, 1]] and got["first_fin_idx"].tolist() == [5, cc.NO_IDX, cc.NO_IDX]
    assert got["flags_or"].tolist() == [0x11, 0, 0] and got["bytes"][2].tolist() == [5, (1 << 64) - 1]
    assert got["bytes"][2, 0] == 5                                       # 0 + 5, and the other side holds 2^64 - 1 alone
    assert_folds_agree(nf, T.records(nf, []))


def test_fold_on_a_seeded_stream_of_the_class(nf):
    recs = cc.seeded_stream(nf.FLOW_RECORD, 3000, 21, 400)
    got = assert_folds_agree(nf, recs)
    assert len(got) > 350 and (got["flows"] > 0).all(axis=1).sum() > 200 and (got["first_fin_idx"] != cc.NO_IDX).sum() > 50
    assert 400 < cc.fold(recs, T.NOW, T.MONO)[2] < 1000
    udp = got[np.isin(got["first_idx"], np.flatnonzero(recs["id"]["transport_protocol"] != 6))]
    assert len(udp) > 100 and (udp["flags_or"] == 0).all() and (udp["first_fin_idx"] == cc.NO_IDX).all()


@pytest.mark.parametrize("now", CLOCKS)
@pytest.mark.parametrize("mono", [T.MONO, 7])
def test_fold_on_the_time_cases(nf, now, mono):
    recs, where = cc.time_stream(nf.FLOW_RECORD, mono)
    got = assert_folds_agree(nf, recs, now, mono)
    assert len(got) == len(where) == 72 and {0, mono, (1 << 64) - 1} <= set(cc.time_values(mono))
    nc = len(where)
    ms = T.maps(recs, now, mono)                                         # flow j of connection c is record j * nc + c
    start = np.array([m[b"TimeFlowStartMs"] for m in ms]).reshape(3, nc)
    end = np.array([m[b"TimeFlowEndMs"] for m in ms]).reshape(3, nc)
    at_min, at_max = np.array([a for a, _ in where]), np.array([b for _, b in where])      # the stream is what it says (ties within one ms aside)
    assert (start[at_min, np.arange(nc)] == start.min(axis=0)).all() and (end[at_max, np.arange(nc)] == end.max(axis=0)).all()
    assert (start.argmin(axis=0) == at_min).sum() > 60 and (end[::-1].argmax(axis=0) == 2 - at_max).sum() > 60
    assert (got["start_ms_min"] == start.min(axis=0)).all() and (got["end_ms_max"] == end.max(axis=0)).all()
    if now < 10**9:
        assert (got["start_ms_min"] < 0).sum() > 20 and (got["end_ms_max"] < 0).sum() >= 18


def test_the_crafted_families_derived_again():
    def total(t):
        fl = {b"SrcAddr": t["src"].encode(), b"SrcPort": t["sport"], b"DstAddr": t["dst"].encode(), b"DstPort": t["dport"], b"Proto": t["proto"]}
        h = CT.compute_hash(fl, T.KD)[2]
        assert "%x" % h == t["total"]
        return h
    assert CRAFTED["searched"] == 1 << 22 and CRAFTED["searched_word0"] == 1 << 25
    assert CRAFTED["candidates"] == dict(same_home=4285, wrap_1024=12304, wrap_8192=1512, same_word0=116)
    same = [total(t) for t in CRAFTED["same_home"]]
    assert len(set(same)) == 200 and {ST.home_slot(h) for h in same} == {CRAFTED["home_slot"]}
    small, big = [total(t) for t in CRAFTED["wrap_1024"]], [total(t) for t in CRAFTED["wrap_8192"]]
    assert len(set(small)) == 40 and all(ST.home_slot(h) >= 1021 for h in small)
    assert len(set(big)) == 30 and all(ST.home_slot(h, 8192) >= 8189 for h in big)
    assert len(CRAFTED["same_word0"]) >= 16
    for a, b in CRAFTED["same_word0"]:
        ta, tb = total(a), total(b)
        assert ta != tb and ta >> 32 == tb >> 32 and ST.home_slot(ta) == ST.home_slot(tb) == a["home"] == b["home"]
    assert len({t["total"] for pair in CRAFTED["same_word0"] for t in pair}) == 2 * len(CRAFTED["same_word0"])
