"""Host-side pieces of the boundary that need no GPU, checked against the oracle:
hashes/sharding, record time derivation (record.go:90-97), the HLL estimator,
the synthetic generators."""
import ctypes as C

import numpy as np
import pytest


def test_key_hash_and_shard_match_oracle(nf, O):
    recs = O.gen_stream(2000, seed=7, n_keys=500, variant=1)      # dirty padding byte 39 included
    for r in recs[:300]:
        kb = r["id"].tobytes()
        assert nf.key_hash(kb) == O.lib().orc_key_hash(kb)
        for n in (1, 2, 3, 8):
            assert nf.shard_of(kb, n) == O.lib().orc_shard_of(kb, n) < n
    # byte 39 is not part of the key (bpf_x86_bpfel.go:119 blank field)
    kb = bytearray(recs[0]["id"].tobytes()); h0 = nf.key_hash(bytes(kb)); kb[39] ^= 0xff
    assert nf.key_hash(bytes(kb)) == h0


def test_ip_hash_matches_oracle(nf, O):
    rng = np.random.default_rng(3)
    for _ in range(200):
        ip = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        for s in range(4):
            assert nf.ip_hash(ip, s) == O.lib().orc_ip_hash(ip, s)


def test_shards_partition_the_population(nf):
    from netobserv_ebpf_agent_amd import synth
    pops = [synth.shard_population(2000, 4, s) for s in range(4)]
    allm = np.concatenate(pops)
    assert len(np.unique(allm)) == len(allm)              # disjoint
    lo = int(min(p.max() for p in pops))
    assert set(range(lo + 1)) <= set(allm.tolist())        # and covering: every member up to the shortest shard's reach


def test_record_times_match_oracle_and_reference_vector(nf, O):
    # account_test.go:104-126: now - (1000-123) ns / now - (1000-789) ns
    now = 1661272402 * 10**9
    m = np.zeros(1, dtype=nf.FLOW_METRICS)
    m["start_mono_time_ts"], m["end_mono_time_ts"] = 123, 789
    s, e = nf.record_times(now, 1000, m[0])
    assert (s, e) == (now - (1000 - 123), now - (1000 - 789))
    rng = np.random.default_rng(5)
    for _ in range(100):
        m["start_mono_time_ts"] = int(rng.integers(0, 2**63)) * 2 + int(rng.integers(0, 2))
        m["end_mono_time_ts"] = int(rng.integers(0, 2**63))
        mono = int(rng.integers(0, 2**63))
        a, b = C.c_int64(0), C.c_int64(0)
        om = m.view(O.FLOW_METRICS)
        O.lib().orc_record_times(now, mono, om.ctypes.data_as(C.c_void_p), C.byref(a), C.byref(b))
        assert nf.record_times(now, mono, m[0]) == (a.value, b.value)     # uint64 wrap included


def test_new_record_mirrors_reference(nf):
    """pkg/model/record.go:82-114 through the host mirror (account_test.go expectations)."""
    r = np.zeros(1, dtype=nf.FLOW_RECORD)[0]
    r["metrics"]["start_mono_time_ts"], r["metrics"]["end_mono_time_ts"] = 123, 789
    r["metrics"]["nb_observed_intf"] = 2
    r["metrics"]["observed_intf"][:2] = [7, 8]
    r["metrics"]["observed_direction"][:2] = [1, 0]
    now = 1661272402 * 10**9
    rec = nf.NewRecord(r["id"], r["metrics"], now, 1000)
    assert rec.TimeFlowStart == now - 877 and rec.TimeFlowEnd == now - 211
    assert [(i.Interface, i.Direction, i.Udn) for i in rec.Interfaces] == [
        ("[namer unset] 0", 0, ""), ("[namer unset] 7", 1, ""), ("[namer unset] 8", 0, "")]


def test_hll_estimator_from_histogram_within_1ulp_of_scalar(nf, O):
    """north_star: HLL estimate agrees with a scalar HLL on the same registers to ±1 ULP."""
    from sketchcraft import seeded_registers
    for p, n, regs in seeded_registers():                   # geometric register values as a real HLL would produce for ~n items
        hist = np.bincount(regs, minlength=65).astype(np.uint32)
        got = nf.hll_estimate_from_histogram(hist, p)
        want = O.hll_estimate(regs, p)
        assert abs(got - want) <= np.spacing(want), (p, n, got, want)
    # empty sketch: linear counting of m zeros -> 0
    assert nf.hll_estimate_from_histogram(np.bincount(np.zeros(1 << 14, dtype=np.uint8), minlength=65), 14) == 0.0


def test_synth_host_generator_matches_oracle_generator(nf, O):
    from netobserv_ebpf_agent_amd import synth
    th_p = synth.zipf_thresholds(1000, 1.1)
    th_o = O.zipf_thresholds(1000, 1.1)
    assert np.array_equal(th_p, th_o)
    pop = synth.shard_population(1000, 2, 1)
    for kw in (dict(variant=0), dict(variant=1), dict(variant=1, hot_permille=900), dict(variant=0, pop_index=pop)):
        a = synth.stream_host(5000, j0=17, seed=42, n_keys=1000, thresholds=th_p, **kw)
        b = O.gen_stream(5000, j0=17, seed=42, n_keys=1000, thresholds=th_o, **kw)
        assert a.tobytes() == b.tobytes(), kw
    # uniform draw (no table)
    assert synth.stream_host(3000, seed=1, n_keys=1000).tobytes() == O.gen_stream(3000, seed=1, n_keys=1000).tobytes()


def test_zipf_stream_shape(O):
    """Zipf(1.1) over 1000 keys: rank 0 gets ~1/H of the records."""
    th = O.zipf_thresholds(1000, 1.1)
    recs = O.gen_stream(200000, seed=2, n_keys=1000, thresholds=th)
    ports = recs["id"]["src_port"].astype(np.int64) - 1024
    h = sum(k ** -1.1 for k in range(1, 1001))
    frac0 = (ports == 0).mean()
    assert abs(frac0 - 1 / h) < 0.01
    assert len(np.unique(ports)) > 900


def test_config1_plumbing_through_oracle(O):
    """BASELINE configs[0]: 10k records, 1k unique keys, CPU only (no GPU): the
    oracle's Accounter, bytes/packets conserved."""
    recs = O.gen_stream(10000, seed=1, n_keys=1000)
    out = O.run_accounter(recs, max_entries=5000)
    assert [r for r, _ in out] == ["closing"]
    ev = out[0][1]
    assert len(ev) == len(np.unique(recs["id"]["src_port"]))
    assert int(ev["metrics"]["bytes"].sum()) == int(recs["metrics"]["bytes"].sum())
    assert int(ev["metrics"]["packets"].sum()) == int(recs["metrics"]["packets"].sum())


def test_oracle_heavy_hitters_against_numpy(O):
    """orc_cm_topk against an independent numpy composition (unique addresses, per-address orc_cm_query, lexsort)."""
    recs = O.gen_stream(20000, seed=6, n_keys=3000, thresholds=O.zipf_thresholds(3000, 1.2), variant=1)
    cm_s, cm_d, _, _ = O.sketches(recs, 4, 10, 10)
    for side, cm, col in ((0, cm_s, "src_ip"), (1, cm_d, "dst_ip")):
        ips = np.unique(recs["id"][col], axis=0)
        est = np.array([O.lib().orc_cm_query(cm.ctypes.data, 4, 10, ip.tobytes()) for ip in ips], dtype=np.uint64)
        order = sorted(range(len(ips)), key=lambda i: (-int(est[i]), ips[i].tobytes()))
        for k in (1, 7, 500, len(ips) + 5):
            got = O.cm_topk(cm, 4, 10, recs, side, k)
            want = order[:k]
            assert len(got) == len(want)
            assert [g["ip"].tobytes() for g in got] == [ips[i].tobytes() for i in want]
            assert [int(g["estimate"]) for g in got] == [int(est[i]) for i in want]


def test_bench_gpus_n_as_a_plain_process_spawns_its_ranks():
    """`python bench.py --gpus N` must not exit with an error when it is not launched by torch.distributed.run (the driver
    ran the N = 1 bench as a plain command): it becomes the launcher of its N ranks, with the contract's own command line."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "3", "--warmup", "1", "--print-spawn"],
                         capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    cmd = out.stdout.split()
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "8", "--steps", "3", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    sys.path.insert(0, root)
    import bench
    a = bench.parse_args(["--gpus", "8"])
    assert bench.resolve_sizes(a, 8) == (125_000_000, 1_250_000)         # BASELINE.json configs[3]: 1 B records, 10 M flows over 8 GPUs
    assert bench.resolve_sizes(bench.parse_args([]), 1) == (100_000_000, 1_000_000)   # configs[1]


def test_bench_stdout_carries_the_json_line_only():
    """bench.py's stdout is the driver's contract: ONE JSON line. Whatever else is written to file descriptor 1 while the bench
    runs (RCCL's banner, a compiler started by ensure_built()) must end up on stderr (bench._QuietStdout)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import os, sys; sys.path.insert(0, %r); import bench\n"
            "q = bench._QuietStdout()\n"
            "print('python-level chatter')\n"
            "os.write(1, b'library-level chatter on fd 1\\n')\n"
            "import subprocess; subprocess.check_call(['echo', 'a child process'])\n"
            "q.emit('{\"value\": 1}')\n"
            "print('after the line')\n") % root
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert p.stdout == '{"value": 1}\n'
    for s in ("python-level chatter", "library-level chatter on fd 1", "a child process", "after the line"):
        assert s in p.stderr


def test_bench_options_and_output_dump(nf, tmp_path, monkeypatch):
    """A plain run measures the headline only (--full is off by default), --steps is the number of timed steps (at least one), and
    --dump-outputs writes the evicted flows key-sorted as exact float64 words: all of them, or the same seeded sample every time."""
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, "", 7, 2)
    assert bench.parse_args(["--full", "--dump-outputs", str(tmp_path)]).full
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
    rng = np.random.default_rng(3)
    recs = np.zeros(1000, dtype=nf.FLOW_RECORD)
    recs.view(np.uint8).reshape(-1, 144)[:] = rng.integers(0, 256, (1000, 144), dtype=np.uint8)
    want = nf.sort_by_key(recs).view(np.uint8).reshape(-1, 144)
    shuffled = recs[rng.permutation(1000)]                       # eviction order is not part of the result
    bench.dump_outputs(str(tmp_path / "all"), "flows", shuffled.view(np.uint8))
    words = np.load(tmp_path / "all" / "flows.npy")
    assert words.dtype == np.float64 and words.shape == (1000, 36)
    assert np.array_equal(words.astype(np.uint32).view(np.uint8).reshape(-1, 144), want)
    assert np.array_equal(np.load(tmp_path / "all" / "flows_index.npy"), np.arange(1000))
    assert np.load(tmp_path / "all" / "flows_count.npy").tolist() == [1000.0]
    monkeypatch.setattr(bench, "DUMP_MAX_FLOWS", 256)
    for d, src in (("s1", shuffled), ("s2", recs)):
        bench.dump_outputs(str(tmp_path / d), "flows", src.view(np.uint8), parts=2)
    idx = np.load(tmp_path / "s1" / "flows_index.npy")
    assert len(idx) == 128 and np.array_equal(idx, np.load(tmp_path / "s2" / "flows_index.npy")) and np.all(np.diff(idx) > 0)
    words = np.load(tmp_path / "s1" / "flows.npy")
    assert np.array_equal(words, np.load(tmp_path / "s2" / "flows.npy"))
    assert np.array_equal(words.astype(np.uint32).view(np.uint8).reshape(-1, 144), want[idx.astype(np.int64)])


def test_bench_line_never_reports_a_fraction_above_one():
    """bench.py frac_of_a_real_bound: SURVEY 8(d)'s algorithmic bytes over the launch time are a model; where the model exceeds the
    peak the line's achieved / frac are those of a real bound (counter traffic if a fresh PMC file exists, else the stream floor)."""
    import bench
    ok = {"achieved": 7800.0, "frac": 0.975, "frac_basis": "alg_model", "alg_model_GBs": 7800.0, "traffic": 4900.0, "frac_traffic": 0.6125,
          "traffic_stale": False, "frac_stream_floor": 0.36}
    assert bench.frac_of_a_real_bound(dict(ok)) == ok                                   # at or below the peak: the contract's definition stands
    over = dict(ok, achieved=8264.7, frac=1.0331, alg_model_GBs=8264.7)
    got = bench.frac_of_a_real_bound(dict(over))
    assert (got["frac"], got["achieved"], got["frac_basis"], got["alg_model_GBs"]) == (0.6125, 4900.0, "counter_traffic", 8264.7)
    stale = bench.frac_of_a_real_bound(dict(over, traffic_stale=True))                 # a traffic file of another build does not count
    assert stale["frac_basis"] == "stream_floor" and stale["frac"] == 0.36 and stale["achieved"] == round(0.36 * bench.HBM_PEAK_GBS, 1)
    none = bench.frac_of_a_real_bound(dict(over, traffic=None, frac_traffic=None))
    assert none["frac_basis"] == "stream_floor" and none["frac"] <= 1.0


def test_account_loop_batching_policy_on_cpu(O):
    """The host loop of the Accounter mirror (netobserv-ebpf-agent_amd/accounter.py Account: the batching policy of INTEGRATION.md
    section 3) with the flow table replaced by the oracle's — TEST scaffolding: the object is put together by hand here, the product's
    constructor knows no table but libnfagg's. What the loop itself must guarantee whatever folds the records (account.go:58-100):
    records received before a tick are accounted before the tick's eviction, closing accounts what was received and then evicts,
    batches are flushed by size and by age, an eviction on full resets the ticker."""
    import queue
    import threading
    import time
    import netobserv_ebpf_agent_amd as nf
    from netobserv_ebpf_agent_amd import accounter as A

    class OracleTable:                                      # the three calls the loop makes, answered by oracle/nfagg_oracle.c
        def __init__(self, max_entries):
            self.acc, self.max_entries = O.Accounter(max_entries, 0), max_entries

        def __len__(self):
            return len(self.acc)

        def account(self, records):
            raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
            n, off, epochs = len(raw) // 144, 0, []
            while off < n:
                off += self.acc.ingest(raw[off * 144:])
                if off < n:
                    epochs.append(self.acc.evict().view(nf.FLOW_RECORD))
            return nf.OK, n, epochs

        def evict(self, code):
            return self.acc.evict().view(nf.FLOW_RECORD)

        def close(self):
            self.acc.close()

    def make(max_entries, evict_timeout, batch_records, batch_timeout):
        a = A.Accounter.__new__(A.Accounter)
        a.maxEntries, a.evictTimeout, a.clock, a.monoClock, a.metrics = max_entries, evict_timeout, (lambda: 10**18), (lambda: 1000), A.NoOp()
        a.batchRecords, a.batchTimeout, a.calls, a.table = batch_records, batch_timeout, 0, OracleTable(max_entries)
        return a

    recs = O.gen_stream(9, seed=3, n_keys=3)                  # three flows, three records each
    one = lambda k: recs[k:k + 1].view(nf.FLOW_RECORD)
    # by size: nothing is handed over before the third record; by age: the rest follows after batch_timeout
    a = make(100, 3600.0, 3, 0.2)
    inp, out = queue.Queue(), queue.Queue()
    th = threading.Thread(target=a.Account, args=(inp, out), daemon=True)
    th.start()
    inp.put(one(0)); inp.put(one(1))
    time.sleep(0.05)
    assert a.calls == 0
    inp.put(one(2))
    time.sleep(0.1)
    assert a.calls == 1 and len(a.table) == 3
    inp.put(one(3))
    time.sleep(0.5)
    assert a.calls == 2                                       # the lone record went after 0.2 s
    inp.put(one(4)); inp.put(A.CLOSE)                         # closing: the record is accounted, then everything is evicted
    batch = out.get(timeout=5)
    th.join(timeout=5)
    assert a.calls == 3 and sum(int(r.Metrics["packets"]) for r in batch) == int(recs["metrics"]["packets"][:5].sum())
    assert a.metrics.evictions_total == {("accounter", "closing"): 1}
    # a tick accounts what waits first; an eviction on full happens at the record that finds the map full
    a = make(2, 0.3, 1000, 30.0)
    inp, out = queue.Queue(), queue.Queue()
    th = threading.Thread(target=a.Account, args=(inp, out), daemon=True)
    th.start()
    for k in range(9):
        inp.put(one(k))
    first = out.get(timeout=5)                                # the tick flushed the nine records: the third flow found the map of 2 full
    assert a.calls == 1 and len(first) == 2
    assert a.metrics.evictions_total.get(("accounter", "full"), 0) >= 1
    inp.put(A.CLOSE)
    rest = []
    while th.is_alive() or not out.empty():
        try:
            rest.append(out.get(timeout=1))
        except queue.Empty:
            pass
    th.join(timeout=5)
    assert sum(int(r.Metrics["packets"]) for b in [first] + rest for r in b) == int(recs["metrics"]["packets"].sum())
