#!/usr/bin/env python3
"""First measurement of the network-events device path (run on the GPU box): nfagg_netev_resolve_device, then
nfagg_encode_flp_json_content_netev_device and nfagg_encode_pb_content_netev_device, on the flows a Zipf(1.1) stream over 10 M
keys evicts (2.86 M), with a network-events part on a random half of them and a cookie table of TABLE_ROWS rows (two thirds
ACLs, every fourth of them dropping). The existing content encoders run on the same records in the same process as the
yardstick. Reported: the median wall time of a whole call and the time per flow / per output byte. Kernel-level device
time: run under rocprofv3 --kernel-trace --stats.

--small: 100 k keys, to check the tool itself."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import netobserv_ebpf_agent_amd as nf  # noqa: E402
from netobserv_ebpf_agent_amd import synth  # noqa: E402

REPS = 5
TABLE_ROWS = 300
FLOWS = 100_000 if "--small" in sys.argv[1:] else 10_000_000
names = nf.intf_table([(2, None, "eth0", ""), (3, None, "eth1", "default"), (4, None, "br-ex", ""), (5, None, "ovn-k8s-mp0", "blue")])
agent = bytes(10) + b"\xff\xff" + bytes([10, 0, 0, 1])
NOW, MONO, RECEIVED = 10**18, 10**12, 1_700_000_000
ACTORS = ["NetworkPolicy", "AdminNetworkPolicy", "EgressFirewall", "NetpolNamespace"]


def timed(fn):
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, float(np.median(ts))


def table_entries():
    out = []
    for k in range(TABLE_ROWS):
        cookie = (0x1000 + 7 * k).to_bytes(8, "little")
        if k % 3 == 2:
            out.append((cookie, b"sample %d of an observability app" % k))
        else:
            action = "drop" if k % 4 == 0 else "allow"
            name, ns = "policy-%d" % k, "namespace-%d" % (k % 17)
            verb = "Dropped" if action == "drop" else "Allowed"
            out.append((cookie, (action, ACTORS[k % 4], name, ns, "Ingress", "%s by %s %s in namespace %s, direction Ingress" % (verb, ACTORS[k % 4], name, ns))))
    return out


def report(what, m, dt, wrote=None):
    tail = f", {wrote} bytes ({wrote / m:.1f} B/flow), {dt / wrote * 1e12:.3f} ps per output byte" if wrote else ""
    print(f"  {what:22s} {m} flows in {dt * 1e3:.3f} ms per call = {dt / m * 1e9:.3f} ns/flow{tail}")


n = 4 * FLOWS
d_th = torch.from_numpy(synth.zipf_thresholds(FLOWS, 1.1).view(np.int64)).cuda()
d = torch.empty(n * 144, dtype=torch.uint8, device="cuda")
synth.stream_device(d.data_ptr(), n, seed=2, n_keys=FLOWS, d_thresholds=d_th.data_ptr())
torch.cuda.synchronize()
with nf.FlowTable(max_entries=FLOWS) as tab:
    rc, consumed = tab.ingest_device(d.data_ptr(), n)
    assert (rc, consumed) == (nf.OK, n), (rc, consumed)
    del d
    d_ev = torch.empty(FLOWS * 144 + 16, dtype=torch.uint8, device="cuda")
    m = tab.evict_device(d_ev.data_ptr(), FLOWS)
    print(f"{FLOWS} keys, {n} records -> {m} evicted flows; table of {TABLE_ROWS} rows")
    entries = table_entries()
    g = torch.Generator(device="cuda").manual_seed(9)
    cookies = torch.from_numpy(np.frombuffer(b"".join(c for c, _ in entries), dtype=np.uint8).reshape(-1, 8).copy()).cuda()
    d_ne = torch.zeros((m, 72), dtype=torch.uint8, device="cuda")
    d_ne[:, 16:48] = cookies[torch.randint(0, TABLE_ROWS, (m, 4), device="cuda", generator=g)].reshape(m, 32)
    d_ne[:, 48:64:2] = torch.randint(1, 200, (m, 8), dtype=torch.uint8, device="cuda", generator=g)      # bytes and packets, 1..199
    d_ne[:, 62] = 0                                                                                       # slot 3 not counted
    d_present = torch.randint(0, 2, (m,), dtype=torch.uint8, device="cuda", generator=g) * nf.FEAT_NETWORK_EVENTS
    d_drops = torch.zeros((m, 32), dtype=torch.uint8, device="cuda")
    d_p_out, d_d_out = torch.empty_like(d_present), torch.empty_like(d_drops)
    d_rows = torch.empty((m, 4), dtype=torch.int16, device="cuda")
    d_set = torch.empty(1024, dtype=torch.int64, device="cuda")
    d_off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
    d_def = torch.empty(m, dtype=torch.uint8, device="cuda")
    d_len = torch.empty(m, dtype=torch.int32, device="cuda")
    with tab.netev_table(entries) as table:
        (n_miss, zero, over), dt = timed(lambda: tab.netev_resolve_device(
            table, d_present.data_ptr(), d_ne.data_ptr(), d_drops.data_ptr(), m, d_p_out.data_ptr(), d_d_out.data_ptr(), d_rows.data_ptr(),
            d_set.data_ptr(), 1024))
        assert n_miss == 0 and not over
        report("resolve", m, dt)
        print(f"  events on {int((d_present != 0).sum())} flows, drops injected on {int(((d_p_out & nf.FEAT_DROPS) != 0).sum())}")
        with tab.netev_table([]) as empty:
            (n_miss, _, over), dt = timed(lambda: tab.netev_resolve_device(
                empty, d_present.data_ptr(), d_ne.data_ptr(), d_drops.data_ptr(), m, d_present.data_ptr(), d_drops.data_ptr(), d_rows.data_ptr(),
                d_set.data_ptr(), 1024))
            assert n_miss == TABLE_ROWS and not over
            report("resolve, empty table", m, dt)
        tab.netev_resolve_device(table, d_present.data_ptr(), d_ne.data_ptr(), d_drops.data_ptr(), m, d_p_out.data_ptr(), d_d_out.data_ptr(),
                                 d_rows.data_ptr(), d_set.data_ptr(), 1024)
        parts = {"drops": d_d_out.data_ptr()}
        # JSON: the existing content encoder on the decorated parts (no events), then the new one
        for what, call in (
                ("json content", lambda out, cap: tab.encode_flp_json_content_device(
                    d_ev.data_ptr(), m, d_p_out.data_ptr(), parts, NOW, MONO, names, agent, RECEIVED, out, cap, d_off.data_ptr(), d_def.data_ptr())),
                ("json content + events", lambda out, cap: tab.encode_flp_json_netev_device(
                    d_ev.data_ptr(), m, d_p_out.data_ptr(), parts, d_rows.data_ptr(), table, NOW, MONO, names, agent, RECEIVED, out, cap,
                    d_off.data_ptr(), d_def.data_ptr()))):
            rc, need, _ = call(0, 0)
            d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
            (rc, wrote, n_def), dt = timed(lambda: call(d_out.data_ptr(), need))
            assert rc == nf.OK and wrote == need and n_def == 0
            report(what, m, dt, wrote)
            del d_out
        for what, call in (
                ("pb content", lambda out, cap: tab.encode_pb_device(
                    d_ev.data_ptr(), m, NOW, MONO, agent, names, out, cap, d_off.data_ptr(), d_len.data_ptr(), d_present=d_p_out.data_ptr(), d_parts=parts)),
                ("pb content + events", lambda out, cap: tab.encode_pb_netev_device(
                    d_ev.data_ptr(), m, d_p_out.data_ptr(), parts, d_rows.data_ptr(), table, NOW, MONO, agent, names, out, cap, d_off.data_ptr(),
                    d_len.data_ptr()))):
            rc, need = call(0, 0)
            d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
            (rc, wrote), dt = timed(lambda: call(d_out.data_ptr(), need))
            assert rc == nf.OK and wrote == need
            report(what, m, dt, wrote)
            del d_out
