#!/usr/bin/env python3
"""Throughput of the device-resident evict -> direct-FLP JSON encode hand-off (nfagg_encode_flp_json_device), with
nfagg_encode_ipfix_device on the same evicted records in the same process as the A/B, and the host path it replaces
(pipeline.DirectFLPStdout: RecordToMap + json.dumps per flow) on a sample of the same flows (run on the GPU box).

Per size: a Zipf(1.1) stream over F keys (4 F records) is folded and evicted on the device; both encoders then run on the
evicted records. Reported per encoder: the median wall time of a whole call (size pass, its read-back of the total,
write pass), flows/s, bytes moved (144 B per flow read, the output bytes written, 8 B per flow of offsets; the JSON
encoder also writes and reads 32 B per flow of interface rows and writes 1 B per flow of deferred flags) and that rate
as a fraction of 8 TB/s. Kernel-level device time: run under rocprofv3 --kernel-trace --stats."""
import io
import os
import queue
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import netobserv_ebpf_agent_amd as nf  # noqa: E402
from netobserv_ebpf_agent_amd import synth  # noqa: E402

HBM = 8e12
REPS = 5
HOST_SAMPLE = 20_000
NAMES = {2: "eth0", 3: "eth1", 4: "br-ex", 5: "ovn-k8s-mp0"}
names = nf.intf_table([(2, None, "eth0", ""), (3, None, "eth1", "default"), (4, None, "br-ex", ""), (5, None, "ovn-k8s-mp0", "blue")])
agent = bytes(10) + b"\xff\xff" + bytes([10, 0, 0, 1])
NOW, MONO = 10**18, 10**12


def timed(fn):
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, float(np.median(ts))


def line(what, m, dt, wrote, extra_per_flow):
    moved = m * (144 + 8 + extra_per_flow) + wrote
    print(f"  {what:6s} {m} flows -> {wrote} bytes ({wrote / m:.1f} B/flow) in {dt * 1e3:.3f} ms = {m / dt / 1e6:.1f} M flows/s, "
          f"{moved / dt / 1e9:.1f} GB/s read+written = {moved / dt / HBM:.3f} of 8 TB/s")
    return dt


for flows in (1_000_000, 10_000_000):
    n = 4 * flows
    d_th = torch.from_numpy(synth.zipf_thresholds(flows, 1.1).view(np.int64)).cuda()
    d = torch.empty(n * 144, dtype=torch.uint8, device="cuda")
    synth.stream_device(d.data_ptr(), n, seed=2, n_keys=flows, d_thresholds=d_th.data_ptr())
    torch.cuda.synchronize()
    with nf.FlowTable(max_entries=flows) as tab:
        rc, consumed = tab.ingest_device(d.data_ptr(), n)
        assert (rc, consumed) == (nf.OK, n), (rc, consumed)
        del d
        d_ev = torch.empty(flows * 144 + 16, dtype=torch.uint8, device="cuda")
        m = tab.evict_device(d_ev.data_ptr(), flows)
        print(f"{flows} keys, {n} records -> {m} evicted flows")
        # direct-FLP JSON
        d_off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
        d_def = torch.empty(m, dtype=torch.uint8, device="cuda")
        rc, need, n_def = tab.encode_flp_json_device(d_ev.data_ptr(), m, NOW, MONO, names, agent, 1_700_000_000, 0, 0, d_off.data_ptr())
        d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
        (rc, wrote, n_def), dt = timed(lambda: tab.encode_flp_json_device(d_ev.data_ptr(), m, NOW, MONO, names, agent, 1_700_000_000,
                                                                          d_out.data_ptr(), need, d_off.data_ptr(), d_def.data_ptr()))
        assert rc == nf.OK and wrote == need and n_def == 0
        dt_json = line("json", m, dt, wrote, 64 + 1)
        del d_out, d_def
        # IPFIX on the same records (A/B)
        rc, need = tab.encode_ipfix_device(d_ev.data_ptr(), m, NOW, MONO, names, 1_700_000_000, 0, 0, 0, d_off.data_ptr())
        d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
        (rc, wrote), dt = timed(lambda: tab.encode_ipfix_device(d_ev.data_ptr(), m, NOW, MONO, names, 1_700_000_000, 0, d_out.data_ptr(),
                                                                need, d_off.data_ptr()))
        assert rc == nf.OK and wrote == need
        line("ipfix", m, dt, wrote, 0)
        del d_out, d_off
        # the path this replaces: NewRecord + RecordToMap + json.dumps per flow on the host, one core
        sample = d_ev[: min(m, HOST_SAMPLE) * 144].cpu().numpy().view(nf.FLOW_RECORD)
        del d_ev
        nf.SetInterfaceNamer(lambda ifx, mac: NAMES.get(ifx, "unknown"))
        t0 = time.perf_counter()
        q = queue.Queue()
        q.put([nf.NewRecord(r["id"], r["metrics"], NOW, MONO) for r in sample]); q.put(nf.CLOSE)
        nf.DirectFLPStdout(io.StringIO(), time_received=1_700_000_000).ExportFlows(q)
        host = (time.perf_counter() - t0) / len(sample)
        print(f"  host   DirectFLPStdout on {len(sample)} of these flows, 1 core of {os.cpu_count()}: {host * 1e6:.1f} us/flow = "
              f"{1 / host / 1e6:.3f} M flows/s; the GPU call is {host / (dt_json / m):.0f} x that rate")
    torch.cuda.empty_cache()
