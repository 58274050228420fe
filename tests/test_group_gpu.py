"""The multi-GPU group (include/nfagg.h nfagg_group_*, csrc/nfagg_api_group.hip) on ONE GPU: several members on device 0
exercise the stable device partition, the routing, per-shard folds, the stop-on-full logic and the sketch merge (local
kernels instead of RCCL when members share a device); a one-member group on a distinct device goes through the RCCL
calls themselves (ncclCommInitAll / ncclAllReduce at N = 1), from Python and from plain C."""
import os
import subprocess

import numpy as np
import pytest

from conftest import assert_records_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "netobserv-ebpf-agent_amd", "lib")


def _zipf(O, n, keys, seed):
    return O.gen_stream(n, seed=seed, n_keys=keys, thresholds=O.zipf_thresholds(keys, 1.1), variant=1)


def reference_group(nf, O, recs, n_shards, max_entries, mode=0):
    """The group's contract restated with the oracle: shard j = nfagg_shard_of(key); one sequential Accounter per shard
    with ceil(max_entries / N) entries; the first record (in arrival order) whose new key finds its shard full stops the
    group, everything is evicted, the stream goes on."""
    share = (max_entries + n_shards - 1) // n_shards
    ids = np.ascontiguousarray(recs["id"])
    base, fn = ids.ctypes.data, O.lib().orc_shard_of
    shard = np.fromiter((fn(base + 40 * i, n_shards) for i in range(len(ids))), dtype=np.int64, count=len(ids))
    out, off = [], 0
    while True:
        accs = [O.Accounter(share, mode) for _ in range(n_shards)]
        stop = len(recs)
        for j in range(n_shards):
            mine = np.nonzero(shard[off:] == j)[0] + off
            c = accs[j].ingest(recs[mine])
            if c < len(mine):
                stop = min(stop, int(mine[c]))
        if stop == len(recs):
            ev = np.concatenate([a.evict() for a in accs])
            out.append(("closing", nf.sort_by_key(ev.view(nf.FLOW_RECORD))))
            return out
        for a in accs:
            a.close()
        accs = [O.Accounter(share, mode) for _ in range(n_shards)]    # redo the epoch up to the stop
        for j in range(n_shards):
            mine = np.nonzero(shard[off:stop] == j)[0] + off
            assert accs[j].ingest(recs[mine]) == len(mine)
        ev = np.concatenate([a.evict() for a in accs])
        out.append(("full", nf.sort_by_key(ev.view(nf.FLOW_RECORD))))
        off = stop


def drive_group(nf, grp, recs, batch):
    out, off, n = [], 0, len(recs)
    while off < n:
        hi = min(n, off + batch)
        while off < hi:
            rc, c = grp.ingest(recs[off:hi])
            off += c
            if rc == nf.FULL:
                out.append(("full", nf.sort_by_key(grp.evict(nf.REASON_FULL))))
    out.append(("closing", nf.sort_by_key(grp.evict(nf.REASON_CLOSING))))
    return out


@pytest.mark.parametrize("n_members", [1, 3, 8])
def test_group_equals_one_accounter_when_nothing_fills(nf, O, n_members):
    """Sharding is invisible in the result: the members' evictions together = the oracle's single Accounter; the merged
    sketches = the oracle's sketches of the whole stream, on every member."""
    recs = _zipf(O, 400_000, 30_000, seed=31)
    with nf.FlowGroup([0] * n_members, max_entries=1 << 20, sketches=nf.SKETCH_CM | nf.SKETCH_HLL, cm_log2_width=14, hll_p=10,
                      staging_records=150_000) as grp:
        assert grp.ingest(recs.view(nf.FLOW_RECORD)) == (nf.OK, len(recs))
        want = O.run_accounter(recs, 1 << 20)[0][1]
        assert len(grp) == len(want)
        grp.merge_sketches()
        cs, cd, hs, hd = O.sketches(recs, 4, 14, 10)
        for m in grp.members:
            assert np.array_equal(m.sketch_snapshot(nf.CM_SRC), cs) and np.array_equal(m.sketch_snapshot(nf.CM_DST), cd)
            assert np.array_equal(m.sketch_snapshot(nf.HLL_SRC), hs) and np.array_equal(m.sketch_snapshot(nf.HLL_DST), hd)
        per_member = [int(m.stats().records_ingested) for m in grp.members]
        assert sum(per_member) == len(recs) and (n_members == 1 or min(per_member) > 0)
        got = nf.sort_by_key(grp.evict(nf.REASON_CLOSING))
    assert_records_equal(got, want)


@pytest.mark.parametrize("n_members,max_entries,batch", [(3, 9_000, 1 << 30), (4, 2_000, 50_000), (2, 16_000, 120_000)])
def test_group_stops_exactly_where_a_shard_fills(nf, O, n_members, max_entries, batch):
    recs = _zipf(O, 300_000, 40_000, seed=32)
    want = reference_group(nf, O, recs, n_members, max_entries)
    assert sum(1 for r, _ in want if r == "full") >= 2
    with nf.FlowGroup([0] * n_members, max_entries=max_entries, staging_records=100_000) as grp:
        got = drive_group(nf, grp, recs.view(nf.FLOW_RECORD), batch)
    assert [(r, len(b)) for r, b in got] == [(r, len(b)) for r, b in want]
    for k, ((_, g), (_, w)) in enumerate(zip(got, want)):
        assert_records_equal(g, w, f"group eviction #{k}")


def test_group_device_resident_input(nf, O):
    import torch
    recs = _zipf(O, 500_000, 50_000, seed=33)
    d = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    with nf.FlowGroup([0, 0, 0, 0], max_entries=1 << 20) as grp:
        for src, (a, b) in enumerate(((0, 200_000), (200_000, 500_000))):
            assert grp.ingest_device(src, d.data_ptr() + a * 144, b - a) == (nf.OK, b - a)
        got = nf.sort_by_key(grp.evict(nf.REASON_CLOSING))
    assert_records_equal(got, O.run_accounter(recs, 1 << 20)[0][1])


@pytest.mark.parametrize("n_members,max_entries,batch", [(3, 1 << 20, 1 << 30), (2, 6_000, 1 << 30), (4, 6_000, 70_000), (8, 1 << 20, 90_000)])
def test_routed_group_in_kernel_dedup_mode(nf, O, n_members, max_entries, batch):
    """NFAGG_MODE_KERNEL_DEDUP across members (BASELINE configs[4] names it for 8 GPUs): routed — every flow on its owner, which
    sees all its records in arrival order (the stable partition keeps it), so the merge of bpf/flows.c:76-143 is exact; buckets
    of 65 536 records or more take the streaming + partition passes, smaller ones the direct kernels. Against the group's
    contract restated with per-shard oracle Accounters in dedup mode, stop-on-full included."""
    from conftest import dedup_stream
    recs = dedup_stream(O, 300_000, seed=47, n_keys=40_000, thresholds=O.zipf_thresholds(40_000, 1.1), style=2)
    want = reference_group(nf, O, recs, n_members, max_entries, mode=1)
    with nf.FlowGroup([0] * n_members, max_entries=max_entries, mode=nf.MODE_KERNEL_DEDUP) as grp:
        got = drive_group(nf, grp, recs.view(nf.FLOW_RECORD), batch)
    assert [r for r, _ in got] == [r for r, _ in want]
    for k, ((_, g), (_, w)) in enumerate(zip(got, want)):
        assert_records_equal(g, w, f"group eviction #{k}")


@pytest.mark.parametrize("local_fold", [False, True])
def test_group_fed_by_one_host_thread_per_source_member(nf, O, local_fold):
    """include/nfagg.h: distinct source members may be fed concurrently. Four threads feed four members with chunk after
    chunk of THEIR OWN flows (thread t owns the flows of key-hash class t of 4, so the order in which concurrent calls are
    served cannot change any flow's result); routed mode partitions the chunks concurrently and folds them one call at a
    time, local-fold mode folds concurrently. Result = ONE Accounter over the stream."""
    import threading
    import torch
    recs = _zipf(O, 1_200_000, 80_000, seed=71)
    cls = nf.distributed.shard_ids(recs.view(nf.FLOW_RECORD), 4)
    parts = [np.ascontiguousarray(recs[cls == t]) for t in range(4)]
    dev = [torch.from_numpy(p.view(np.uint8).reshape(-1).copy()).cuda() for p in parts]
    torch.cuda.synchronize()
    errors = []
    with nf.FlowGroup([0, 0, 0, 0], max_entries=1 << 20, local_fold=local_fold, sketches=nf.SKETCH_CM, cm_log2_width=12) as grp:
        def feed(t):
            try:
                off, n = 0, len(parts[t])
                while off < n:
                    c = min(n - off, 37_000 + 5_000 * t)
                    rc, took = grp.ingest_device(t, dev[t].data_ptr() + off * 144, c)
                    assert (rc, took) == (nf.OK, c), (t, off, rc, took)
                    off += c
            except BaseException as exc:       # surfaced in the main thread
                errors.append(exc)
        ths = [threading.Thread(target=feed, args=(t,)) for t in range(4)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errors, errors
        assert sum(m.stats().records_ingested for m in grp.members) == len(recs)
        got = nf.sort_by_key(grp.evict(nf.REASON_CLOSING))
    assert_records_equal(got, O.run_accounter(recs, 1 << 20)[0][1])


def test_one_member_group_goes_through_rccl(nf, O):
    """Distinct devices -> the RCCL path (communicator + all-reduce), here with the one GPU the box has."""
    recs = _zipf(O, 100_000, 5_000, seed=34)
    with nf.FlowGroup([0], max_entries=1 << 16, sketches=nf.SKETCH_CM | nf.SKETCH_HLL, cm_log2_width=12, hll_p=10) as grp:
        assert grp.ingest(recs.view(nf.FLOW_RECORD)) == (nf.OK, len(recs))
        grp.merge_sketches()
        cs, _, hs, _ = O.sketches(recs, 4, 12, 10)
        assert np.array_equal(grp.members[0].sketch_snapshot(nf.CM_SRC), cs)
        assert np.array_equal(grp.members[0].sketch_snapshot(nf.HLL_SRC), hs)
        assert_records_equal(nf.sort_by_key(grp.evict(nf.REASON_CLOSING)), O.run_accounter(recs, 1 << 16)[0][1])


@pytest.fixture(scope="module")
def group_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gdriver") / "nfagg_group_cdriver")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "c", "nfagg_group_cdriver.c"), "-o", exe, "-L", LIBDIR, "-lnfagg", "-Wl,-rpath," + LIBDIR])
    return exe


@pytest.mark.parametrize("devices,max_entries", [("0", 1 << 16), ("0,0,0", 3_000)])
def test_group_from_plain_c(nf, O, group_driver, tmp_path, devices, max_entries):
    """No Python, no torch in the process: what the cgo shim of the one-process agent sees. "0" = the RCCL
    path at N = 1 (librccl loaded by the library itself)."""
    recs = _zipf(O, 150_000, 4_000, seed=35)
    src = tmp_path / "records.bin"
    recs.tofile(src)
    out = subprocess.check_output([group_driver, str(src), str(tmp_path / "out"), str(max_entries), "60000", devices], text=True).split("\n")
    n_members = len(devices.split(","))
    want = reference_group(nf, O, recs, n_members, max_entries)
    lines = [l.split() for l in out if l.startswith(("full ", "closing "))]        # RCCL prints its version banner on stdout too
    assert [(r, len(b)) for r, b in want] == [(l[0], int(l[1])) for l in lines]
    got = np.fromfile(tmp_path / "out.records", dtype=O.FLOW_RECORD)
    pos = 0
    for reason, b in want:
        assert_records_equal(nf.sort_by_key(got[pos:pos + len(b)].view(nf.FLOW_RECORD)), b, reason)
        pos += len(b)
    if not any(r == "full" for r, _ in want):                      # sketches see every record of the last epoch... all of them here
        est = float([l for l in out if l.startswith("hll_src")][0].split()[1])
        _, _, hs, _ = O.sketches(recs, 4, 20, 14)
        assert abs(est - O.hll_estimate(hs, 14)) <= np.spacing(est)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_group_randomised_against_the_contract(nf, O, seed):
    """Random member counts, capacities (down to a handful of flows per shard: several shards fill inside one call, claims get
    refused in the smallest tables), batch cuts and staging sizes; every eviction compared with the per-shard-oracle contract."""
    rng = np.random.default_rng(seed)
    n_members = int(rng.choice([1, 2, 3, 5, 8]))
    keys = int(rng.choice([40, 2_000, 30_000]))
    n = int(rng.choice([30_000, 120_000, 250_000]))
    max_entries = int(rng.choice([n_members * 3, max(n_members, keys // 4), keys // 2 + 7, 1 << 20]))
    if max_entries < keys // 8:
        n = min(n, 40_000)                                            # bounded number of eviction round trips
    s = float(rng.choice([0.0, 1.1]))
    th = O.zipf_thresholds(keys, s) if s > 0 else None
    recs = O.gen_stream(n, seed=int(rng.integers(1, 1 << 30)), n_keys=keys, thresholds=th, hot_permille=int(rng.choice([0, 900])), variant=1)
    want = reference_group(nf, O, recs, n_members, max_entries)
    with nf.FlowGroup([0] * n_members, max_entries=max_entries, staging_records=int(rng.choice([0, 1 << 14, 1 << 16]))) as grp:
        got = drive_group(nf, grp, recs.view(nf.FLOW_RECORD), int(rng.choice([1 << 30, 50_000, 7_777])))
    assert [(r, len(b)) for r, b in got] == [(r, len(b)) for r, b in want], dict(seed=seed, n_members=n_members, keys=keys, n=n, max_entries=max_entries)
    for k, ((_, g), (_, w)) in enumerate(zip(got, want)):
        assert_records_equal(g, w, f"seed {seed}, eviction #{k}")
