"""Conversation tracking on the GPU (csrc/nfagg_conn.hip) through the C ABI: partials and hash ids against a per-flow group-by
of the restatement (tests/conntrack_ref.py) on the seeded stream of test_flp_json_gpu.py, through the host and the device entry
point; streams built for the edges (three interfaces, two spellings of one address, src == dst, 5 000 flows of one
connection, the cap and one below it, a cap above the maximum); the crafted table collisions of
tests/golden/conntrack_collisions.json in both arrival orders; and ConnTrack.extract over four calls against the restatement.

The collisions here are folded by one wave of one workgroup. tests/test_crafted_conntrack_gpu.py has the contended cases: crafted
homes and first key words scattered over seven workgroups, probe chains that wrap, full tables, a table above 2^20 slots, the wave
ballots' lane patterns, and other clocks than this file's one."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conntrack_ref as CT  # noqa: E402
import conntrack_streams as ST  # noqa: E402
import test_conntrack_cpu as T  # noqa: E402
import test_flp_json_gpu as J  # noqa: E402
import test_netev_gpu as E  # noqa: E402

pytestmark = pytest.mark.gpu

COLLISIONS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conntrack_collisions.json")))


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


def by_first(parts):
    return parts[np.argsort(parts["first_idx"], kind="stable")]


def fold_both(nf, tab, recs, cap=4096, now=T.NOW, mono=T.MONO):
    """The host call, then the device call into a buffer of exactly the cap with 0xAB canaries over it and 128 bytes behind.
    Both must agree; returns (rc, partials by first_idx, n_conns, hash ids, n_discarded)."""
    import torch
    n = len(recs)
    rc, parts, n_conns, ids, n_disc = tab.conn_fold(recs, now, mono, cap=cap)
    d_recs = E.dev(recs) if n else None
    d_ids = torch.full((n * 8 + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    d_out = torch.full((cap * 128 + 128,), 0xAB, dtype=torch.uint8, device="cuda")
    rc_d, n_conns_d, n_disc_d = tab.conn_fold_device(d_recs.data_ptr() if n else 0, n, now, mono, d_ids.data_ptr(), cap, d_out.data_ptr())
    torch.cuda.synchronize()
    assert (rc_d, n_disc_d) == (rc, n_disc)
    assert n_conns_d == n_conns if rc == nf.OK else (n_conns > cap and n_conns_d > cap)
    raw, raw_ids = d_out.cpu().numpy(), d_ids.cpu().numpy()
    used = n_conns * 128 if rc == nf.OK else 0
    assert (raw[used:] == 0xAB).all(), "bytes behind the partials were written"
    assert (raw_ids[n * 8:] == 0xAB).all() and raw_ids[:n * 8].copy().view(np.uint64).tolist() == ids.tolist()
    got = by_first(raw[:used].copy().view(nf.CONN_PARTIAL))
    assert got.tobytes() == by_first(parts).tobytes()
    return rc, got, n_conns, ids, n_disc


def check_fold(nf, tab, recs, cap=4096, now=T.NOW, mono=T.MONO):
    parts, ids, n_disc = CT.fold(T.maps(recs, now, mono), T.KD)
    rc, got, n_conns, got_ids, got_disc = fold_both(nf, tab, recs, cap, now, mono)
    assert (rc, n_conns, got_disc) == (nf.OK, len(parts), n_disc)
    assert got_ids.tolist() == ids
    want = T.partial_array(nf, parts)
    if got.tobytes() != want.tobytes():
        k = next(i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes())
        raise AssertionError("partial %d:\n got %r\nwant %r" % (k, got[k], want[k]))
    assert len(np.unique(got["first_idx"])) == len(got) and (got["pad_"] == 0).all()
    return got


def seeded(nf, O, n, seed):
    recs = J.stream(nf, O, n, seed)
    if n:
        recs["metrics"]["bytes"] = np.minimum(recs["metrics"]["bytes"], 1 << 40)      # sums stay below 2^53
    return recs


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 513, 4097])
def test_partials_and_hash_ids_on_the_seeded_stream(nf, O, tab, n):
    got = check_fold(nf, tab, seeded(nf, O, n, 5 + n))
    if n >= 513:
        assert len(got) > 50 and (n < 4097 or (got["flows"].sum(axis=1) > 1).any())


def both_ways(flows):
    return [dict(f, src=f["dst"], sport=f["dport"], dst=f["src"], dport=f["sport"]) if k % 2 else f for k, f in enumerate(flows)]


def test_both_directions_on_three_interfaces(nf, tab):
    f = dict(src="10.0.0.1", sport=40000, dst="10.0.0.2", dport=443, proto=6, bytes=1000, packets=3, flags=0x10)
    recs = T.records(nf, both_ways([f] * 6))
    recs["metrics"]["if_index_first_seen"] = [1, 1, 2, 2, 3, 3]
    got = check_fold(nf, tab, recs)
    assert len(got) == 1 and got["flows"].tolist() == [[3, 3]] and got["bytes"].tolist() == [[3000, 3000]]


def test_two_spellings_of_one_address_and_src_equal_dst(nf, tab):
    flows = [dict(src="192.168.1.10", sport=500, dst="192.168.1.11", dport=600, proto=17, bytes=10, packets=1),
             dict(src="::ffff:192.168.1.10", sport=500, dst="::ffff:192.168.1.11", dport=600, proto=17, bytes=20, packets=1),   # an IPv6 record, v4-mapped
             dict(src="::1", sport=8080, dst="::1", dport=8080, proto=6, bytes=5, packets=1),
             dict(src="::1", sport=8080, dst="::1", dport=8080, proto=6, bytes=7, packets=2, flags=0x11),
             dict(src="2001:db8::1", sport=1, dst="2001:db8::2", dport=2, proto=132, bytes=0, packets=0)]
    got = check_fold(nf, tab, T.records(nf, flows))
    assert len(got) == 3 and got["flows"].tolist() == [[2, 0], [2, 0], [1, 0]]          # net.IP prints both spellings alike; hashA == hashB is "same"
    assert got["first_fin_idx"].tolist() == [nf._lib.CONN_NO_IDX, 3, nf._lib.CONN_NO_IDX]


def test_five_thousand_flows_of_one_connection(nf, tab):
    f = dict(src="10.0.0.1", sport=40000, dst="10.0.0.2", dport=443, proto=6, bytes=(1 << 40) - 1, packets=7, flags=0x10)
    recs = T.records(nf, both_ways([f] * 5000))
    recs["metrics"]["flags"][[1234, 4321]] = 0x11
    recs["metrics"]["flags"][77] = 0x100
    got = check_fold(nf, tab, recs)
    assert len(got) == 1
    p = got[0]
    assert (p["first_idx"], p["last_idx"], p["first_fin_idx"], p["flags_or"]) == (0, 4999, 1234, 0x111)
    assert p["flows"].tolist() == [2500, 2500] and p["bytes"].tolist() == [2500 * ((1 << 40) - 1)] * 2


def distinct(nf, n):
    recs = T.records(nf, [dict(src="10.0.0.1", sport=0, dst="10.0.0.2", dport=443, proto=6, bytes=1, packets=1)] * n)
    recs["id"]["src_port"] = 1024 + np.arange(n)
    return recs


def test_the_cap_and_one_below_it(nf, tab):
    recs = distinct(nf, 4096)
    assert len(check_fold(nf, tab, recs, cap=4096)) == 4096
    rc, got, n_conns, ids, n_disc = fold_both(nf, tab, recs, cap=4095)               # fold_both: `out` untouched, a lower bound above the cap
    assert rc == nf.TRUNCATED and len(got) == 0 and n_conns > 4095 and n_disc == 0
    assert ids.tolist() == CT.fold(T.maps(recs), T.KD)[1]                            # hash_ids is still complete
    recs[7]["id"]["transport_protocol"] = 1                                          # one flow fewer is tracked: 4 095 connections fit
    assert len(check_fold(nf, tab, recs, cap=4095)) == 4095


def test_a_cap_above_the_maximum(nf, tab):
    with pytest.raises(nf.NfaggError) as e:
        tab.conn_fold_device(0, 0, T.NOW, T.MONO, 0, nf._lib.CONN_MAX_CONNS + 1, 0)
    assert e.value.code == nf._lib.ERANGE
    out = np.zeros(1, dtype=nf.CONN_PARTIAL)
    n1, n2 = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    opt = nf._lib.ConnOptions(struct_size=24, now_unix_ns=T.NOW, mono_now_ns=T.MONO)
    import ctypes as C
    rc = nf._lib.lib.nfagg_conn_fold(tab._h, None, 0, C.byref(opt), None, nf._lib.CONN_MAX_CONNS + 1, out.ctypes.data_as(C.c_void_p),
                                     n1.ctypes.data_as(C.POINTER(C.c_uint32)), n2.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == nf._lib.ERANGE


# ---- crafted table collisions
def collision_flows(tuples):
    flows = []
    for k, t in enumerate(tuples):
        f = dict(src=t["src"], sport=t["sport"], dst=t["dst"], dport=t["dport"], proto=t["proto"], bytes=100 + k, packets=1 + k, flags=0x10)
        flows += [f, dict(f, src=f["dst"], sport=f["dport"], dst=f["src"], dport=f["sport"], bytes=7)]
    return flows


@pytest.mark.parametrize("reverse", [False, True])
def test_twenty_connections_with_one_home_slot(nf, tab, reverse):
    tuples = COLLISIONS["same_home"]
    assert len(tuples) == 20 and COLLISIONS["searched"] == 1 << 22
    assert {ST.home_slot(int(t["total"], 16)) for t in tuples} == {COLLISIONS["home_slot"]}
    flows = collision_flows(tuples)
    got = check_fold(nf, tab, T.records(nf, flows[::-1] if reverse else flows), cap=64)      # the smallest table: 1 024 slots
    assert len(got) == 20 and sorted("%x" % h for h in got["hash_total"]) == sorted(t["total"] for t in tuples)


@pytest.mark.parametrize("reverse", [False, True])
def test_connections_that_share_the_first_key_word(nf, tab, reverse):
    pairs = COLLISIONS["same_word0"]
    assert pairs and all(int(a["total"], 16) >> 32 == int(b["total"], 16) >> 32 and a["total"] != b["total"] for a, b in pairs)
    # ... and the home slot: whichever of a pair comes second finds word 0 of its home slot equal to its own and word 1 another's
    assert all(ST.home_slot(int(a["total"], 16)) == ST.home_slot(int(b["total"], 16)) == a["home"] for a, b in pairs)
    flows = collision_flows([t for pair in pairs for t in pair])
    got = check_fold(nf, tab, T.records(nf, flows[::-1] if reverse else flows), cap=64)
    assert len(got) == 2 * len(pairs)


# ---- ConnTrack.extract
def test_extract_over_four_calls_against_the_restatement(nf, tab):
    """600 flows in four calls with a moving clock; all four record types, two scheduling groups, and a connection limit below
    the stream's connection count."""
    rng = np.random.default_rng(9)
    ends = [("10.0.%d.%d" % (k // 8, k % 8 + 1), 1000 + k) for k in range(24)] + [("2001:db8::%x" % k, 80 + 100 * k) for k in range(1, 17)]
    cfg = T.config(max_conns=60, flow_logs=True)
    ref, mir = CT.ConnTrack(cfg), nf.ConnTrack(cfg)
    now, seen, kinds = 0, set(), set()
    for call in range(4):
        flows = []
        for _ in range(150):
            lo, n_ends = (0, 24) if rng.integers(0, 2) else (24, 16)
            a, b = rng.choice(n_ends, 2, replace=False)
            flows.append(dict(src=ends[lo + a][0], sport=ends[lo + a][1], dst=ends[lo + b][0], dport=ends[lo + b][1],
                              proto=int(rng.choice([6, 6, 6, 17, 17, 132, 1])), bytes=int(rng.integers(0, 1 << 40)) * int(rng.integers(0, 4) > 0),
                              packets=int(rng.integers(0, 1000)), flags=int(rng.choice([0, 0x10, 0x10, 0x11, 0x112, 0x01, 0x02]))))
        now += int(rng.integers(2 * 10**9, 5 * 10**9))
        recs = T.records(nf, flows)
        ms = T.maps(recs)
        want = [T.norm(r) for r in ref.extract(ms, now)]
        got = mir.extract(tab, recs, now, T.NOW, T.MONO, cap=64, flow_maps=[T.norm(m) for m in ms])      # cap 64: extract grows it
        assert got == want, "call %d" % call
        seen |= {r["_HashId"] for r in want if r["_RecordType"] == "flowLog"}
        kinds |= {r["_RecordType"] for r in want}
    assert kinds == {"newConnection", "endConnection", "heartbeat", "flowLog"} and len(seen) > 60 and len(mir) == len(ref.group_of)
