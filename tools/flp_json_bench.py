#!/usr/bin/env python3
"""Throughput of the device-resident evict -> direct-FLP JSON encode hand-off (nfagg_encode_flp_json_device), with
nfagg_encode_ipfix_device on the same evicted records in the same process as the A/B, and the host path it replaces
(pipeline.DirectFLPStdout: RecordToMap + json.dumps per flow) on a sample of the same flows (run on the GPU box).

Per size: a Zipf(1.1) stream over F keys (4 F records) is folded and evicted on the device; both encoders then run on the
evicted records. Reported per encoder: the median wall time of a whole call (size pass, its read-back of the total,
write pass), flows/s, bytes moved (144 B per flow read, the output bytes written, 8 B per flow of offsets; the JSON
encoder also writes and reads 32 B per flow of interface rows and writes 1 B per flow of deferred flags) and that rate
as a fraction of 8 TB/s. Kernel-level device time: run under rocprofv3 --kernel-trace --stats.

--content: the MapTracer leg instead. The flows evicted at the larger size are encoded as full BpfFlowContents
(nfagg_encode_flp_json_content_device) with every feature part present on about half of them, and as plain records
(nfagg_encode_flp_json_device) in the same process as the yardstick; both report their time per output byte.

--tls: the TLS-name leg. The flows evicted at the larger size are encoded twice in one process: with their TLS fields clear
through nfagg_encode_flp_json_device, the yardstick, then with ssl_version / tls_cipher_suite / tls_key_share set on a seeded
half of them (known and unknown ids, the mismatch flag on some) through nfagg_encode_flp_json_tls_device with the default
name table. Both report their time per flow and per output byte.

--k8s: the Kubernetes leg, at both sizes. The evicted flows are encoded through nfagg_encode_flp_json_tls_device, the yardstick,
and through nfagg_encode_flp_json_k8s_device with a table of 100 000 rows and a layer: every other distinct address of the
evicted flows (as many as fit), filled up with addresses no flow has. The hash join alone (nfagg_k8s_resolve_device) is timed
too. Kernel-level device time: run the same leg under rocprofv3 --kernel-trace --output-format csv -d DIR, then
--k8s-trace DIR prints the median device time of every encoder kernel per launch size from that trace.

--net (with --k8s): the transform network leg on top, on the same records and the same Kubernetes table in the same run:
nfagg_encode_flp_json_net_device with reinterpret_direction, add_subnet_label and decode_tcp_flags on and 48 CIDRs in seven categories
(46 narrow ones no address need match, then 0.0.0.0/0 and ::/0, so that every address walks the whole list). The join alone
(nfagg_net_resolve_device) is timed too; --k8s-trace covers the k_net_* kernels.

--metrics (with --k8s --net): the flow metrics leg on top, on the same records, rows and net rows in the same run:
nfagg_metrics_fold_device with two groupings, the namespace pair + layer + both subnet labels, and owner / type / namespace of both sides
+ direction. Reported: the median wall time of a whole call (the memset of the tables, fold, count, scan, emit, the read-back), the
group counts, the bytes a flow's lane reads by this tool's own count, and that read rate as a fraction of a read-stream rate measured in
the same run (a sum over 1 GiB). --k8s-trace covers the k_metrics_* kernels and the memset's fill kernel.

--content (with --k8s --net --metrics): the content metrics leg on top, on the same records, rows and net rows in the same run:
nfagg_metrics_fold_content_device with synthetic feature parts on about half of the flows and three groupings shaped like the
operator's: the namespace pair + an RTT histogram of ten bounds, the namespace pair + the response code + a DNS-latency histogram,
the namespace pair + drop cause + drop state with both drop sums. It prints beside the plain --metrics leg's time; that time and the
read-stream rate are what its number is read against. NFAGG_LIB selects the library, so a build with another LDS table size
(-DNFAGG_METC_LDS_SLOTS) is measured by a second process of the same command.

--conntrack (with --k8s --net --metrics): the conversation fold on top, on the same records in the same run, beside the plain metrics
fold: nfagg_conn_fold_device with hash ids. Reported: the median wall time of a whole call (the memset of the table, claim, finish,
count, scan, emit, the read-back), the connections and the discarded flows, and the bytes a flow's lanes read and write by this
tool's own count. --k8s-trace covers the k_conn_* kernels. The flow logs follow on the same records and ids in the same run:
nfagg_encode_flp_json_conn_device with the tables of the --net leg, whose _net line above is what its time per output byte is read
against; --k8s-trace covers its kernels (k_flp_* over FlpConnMeta). Then the conversation records, one per connection of the fold
(nfagg_encode_conn_json_device, seven output fields of which two are split): each connection's first flow as its carrier, the
partial's sums as its values; --k8s-trace covers the k_conn_json_* kernels (they match k_conn_).

--filter (with --k8s --net): the transform filter leg on top, on the same records, rows and tables in the same run: a keep_entry_query
of three atoms, (SrcPort < p or DstPort < q) and with(Bytes), with p the median source port and q the 0.3 quantile of the destination ports of the evicted flows, so that about
half of the flows stay, once without sampling and once with keepEntrySampling 10 and samplingField Sampling. Reported: the median wall
time of nfagg_filter_apply_device (eval, the scan, the read-back of the count, the compaction with its records), of the two
nfagg_gather_device calls for the Kubernetes rows and the net rows, and of nfagg_encode_flp_json_net_device on the kept flows, beside
the unfiltered _net call and the net join of the same run; the bytes a flow moves by this tool's own count as a fraction of the
read-stream rate measured in the same run. --k8s-trace covers the k_filter_* and k_gather kernels.

--loki (with --k8s --net --metrics --conntrack): the write loki leg on top, on the same records, tables and hash ids in the same run,
beside the _conn call: the operator's label set (namespace, owner name and owner kind of both sides, K8S_FlowLayer, FlowDirection,
_RecordType), TimeFlowEndMs at a scale of 1ms, at batch sizes of 100 KiB and 10 MiB. Reported per batch size: the median wall time of
nfagg_loki_plan_device, of rendering the streams' label texts on the host (once per stream), of nfagg_loki_write_device, and their sum
(the whole call), with the streams, groups, batches and bytes; the yardstick is the _conn call plus the host loop it replaces.
--k8s-trace covers the k_loki_* kernels, the cut walk (k_loki_cuts) among them. --flows N runs one table size instead of the two.

--ipfix (with --k8s --net): the write ipfix leg on top, on the same records, Kubernetes rows and entries in the same run, beside the
_net call: nfagg_flp_ipfix_write_device with enterprise id 2 and a TCP-sized message limit, the strings table over the leg's 100 000
entries, and nfagg_encode_ipfix_device (the agent's own exporter, 19 fixed fields, no state) on the same records. Reported: the median
wall time of a whole call (presence and carry, the scan over blocks, size, the two scans, the read-back, write, state export), the sent
and failed flows, the bytes, and the bytes a flow moves by this tool's own count. --k8s-trace covers the k_ipfix_* kernels.

--timebased (with --k8s --net --metrics --conntrack): the extract timebased leg on top, on the same records and Kubernetes rows in
the same run, beside the metrics fold and the conversation fold: two rules, the SrcAddr top-10 sum of Bytes and the
SrcK8S_Namespace,DstK8S_Namespace top-10 sum of Bytes, with a window that holds 12 calls. Twelve calls fill the window; then the median
wall time of a whole nfagg_timebased_extract_device call in the steady state (presence, its read-back, claim, fold, finish, the second
read-back, the slice emit, per rule the merges of 12 slices, value, select and sort, the synchronisation, the trim) and of
nfagg_timebased_results_device alone (the evaluation without a new slice). Flows without Bytes are dropped first, as the stage's
caller must. --k8s-trace covers the k_tb_* kernels."""
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
CONTENT = "--content" in sys.argv[1:]
TLS = "--tls" in sys.argv[1:]
K8S = "--k8s" in sys.argv[1:]
NET = "--net" in sys.argv[1:]
METRICS = "--metrics" in sys.argv[1:]
CONNTRACK = "--conntrack" in sys.argv[1:]
FILTER = "--filter" in sys.argv[1:]
LOKI = "--loki" in sys.argv[1:]
IPFIX = "--ipfix" in sys.argv[1:]
TIMEBASED = "--timebased" in sys.argv[1:]
if TIMEBASED and not (K8S and NET and METRICS and CONNTRACK):
    sys.exit("--timebased runs behind --k8s --net --metrics --conntrack: give them too")
FLOWS = int(sys.argv[sys.argv.index("--flows") + 1]) if "--flows" in sys.argv[1:] else 0
NET_CATEGORIES = [("cat-%d" % c, ["172.%d.%d.0/24" % (16 + c, k) for k in range(8)] + ["2001:db8:%x::/48" % (16 * c + k) for k in range(1)]) for c in range(5)] + \
                 [("pods", ["100.64.0.0/10"]), ("everything", ["0.0.0.0/0", "::/0"])]
K8S_ROWS = 100_000
PART_BYTES = {"additional": 32, "dns": 64, "drops": 32, "xlat": 56, "quic": 24}


def device_parts(m, seed=5):
    """present and the five part arrays for m flows, made on the device: all five parts on a random half of the flows, none on
    the others; random bytes, then the fields that gate keys set so that every key appears (a DNS id and a three-label name, a
    core drop cause, v4-mapped xlat addresses, an IPsec return code of zero)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    parts = {k: torch.randint(0, 256, (m, b), dtype=torch.uint8, device="cuda", generator=g) for k, b in PART_BYTES.items()}
    name = np.zeros(32, dtype=np.uint8)
    raw = b"\x03www\x07example\x03com"
    name[: len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    parts["dns"][:, 31:63] = torch.from_numpy(name).cuda()
    parts["dns"][:, 24] |= 1                                          # id != 0
    parts["dns"][:, 21:24] = 0                                        # latency below 2^40 ns
    parts["drops"][:, 20:24] = 0
    parts["drops"][:, 20] = 2 + torch.randint(0, 79, (m,), dtype=torch.uint8, device="cuda", generator=g)
    v4 = torch.from_numpy(np.frombuffer(bytes(10) + b"\xff\xff", dtype=np.uint8).copy()).cuda()
    parts["xlat"][:, 16:28] = v4
    parts["xlat"][:, 32:44] = v4
    parts["xlat"][:, 28] |= 1
    parts["xlat"][:, 44] |= 1
    parts["additional"][:, 21:28] = 0                                 # rtt below 2^40 ns, ipsec_encrypted_ret = 0
    parts["quic"][:, 17:20] = 0
    present = torch.randint(0, 2, (m,), dtype=torch.uint8, device="cuda", generator=g) * 0x37
    torch.cuda.synchronize()
    return present, parts


def set_tls_fields(d_ev, m, seed=7):
    """ssl_version @132, tls_cipher_suite @134, tls_key_share @136, misc_flags @139 of the evicted records in HBM, on a seeded
    half of the flows: ids the default table knows and ids it does not, the mismatch flag on a quarter of that half."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    pick = lambda values: torch.tensor(values, dtype=torch.int64, device="cuda")[torch.randint(0, len(values), (m,), device="cuda", generator=g)]  # noqa: E731
    on = torch.randint(0, 2, (m,), device="cuda", generator=g) == 1
    v = d_ev[: m * 144].view(m, 144)
    for col, values in ((132, [0x0303, 0x0304, 0x0304, 0x0200]), (134, [0x1301, 0x1302, 0xc02f, 0xcca8, 0x00ff]), (136, [29, 23, 4588, 0, 30])):
        w = torch.where(on, pick(values), torch.zeros(m, dtype=torch.int64, device="cuda"))
        v[:, col] = (w & 0xff).to(torch.uint8)
        v[:, col + 1] = (w >> 8).to(torch.uint8)
    v[:, 139] |= (on & (torch.randint(0, 4, (m,), device="cuda", generator=g) == 0)).to(torch.uint8)
    torch.cuda.synchronize()
    return int(on.sum())


def k8s_entries(d_ev, m):
    """K8S_ROWS informer answers: every other distinct address of the m evicted flows' IP records, as many as fit, then
    addresses no flow has. Returns (entries, distinct addresses, flows that are IP)."""
    recs = d_ev[: m * 144].cpu().numpy().view(nf.FLOW_RECORD)
    ip = np.isin(recs["metrics"]["eth_protocol"], (0x0800, 0x86DD))
    both = np.concatenate([recs["id"]["src_ip"][ip], recs["id"]["dst_ip"][ip]])
    distinct = np.unique(np.ascontiguousarray(both).view("V16").reshape(-1))
    take = [a.tobytes() for a in distinct[::2][:K8S_ROWS]]
    fill = [b"\xfd\x00" + bytes(10) + k.to_bytes(4, "big") for k in range(K8S_ROWS - len(take))]
    info = lambda k: dict(namespace="openshift-dns" if k % 10 == 0 else "ns-%d" % (k % 50), name="pod-%d" % k, kind="Pod",  # noqa: E731
                          owner_name="deploy-%d" % (k % 5000), owner_kind="Deployment", network_name="primary", host_ip="10.0.0.%d" % (k % 200),
                          host_name="node-%d" % (k % 200), zone="zone-%s" % "abc"[k % 3])
    return [(a, info(k)) for k, a in enumerate(take + fill)], len(distinct), int(ip.sum())


def k8s_trace(root):
    """Median device time per (kernel, launch size) of the encoder kernels in a rocprofv3 kernel trace below `root`."""
    import csv
    import glob
    import re
    spans = {}
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"]
            if not re.search(r"k_flp_|k_k8s_|k_net_|k_metrics_|k_conn_|k_filter_|k_gather|k_loki_|k_ipfix_|k_tb_|fillBuffer|scan|[Ss]ort|onesweep", name):
                continue
            short = re.sub(r"^void nfagg::|\(.*$|nfagg::", "", name)
            if "rocprim" in name:                           # the library's scan and sort kernels: their configuration's name and value types
                m = re.search(r"wrapped_(\w+?)_config<.*?, (unsigned \w+(?:, unsigned \w+)?)>", name) or re.search(r"detail::(\w+?)<", name)
                short = "rocprim " + " ".join(m.groups()) if m else "rocprim"
            grid = int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0)
            spans.setdefault((short, grid), []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    print("device time per launch from the kernel trace, median over the launches of one size, us:")
    for (short, grid), tv in sorted(spans.items(), key=lambda kv: (kv[0][1] > 4_000_000, kv[0][0], kv[0][1])):
        v = [us for _, us in tv]
        print(f"  {short:48s} grid {grid:9d}: {float(np.median(v)):9.1f}  min {min(v):9.1f}  max {max(v):9.1f}  ({len(v)} launches)")
    # the conversation table's memset is among the many fills of one grid: the longest fills, which are the largest tables'
    for (short, grid), tv in sorted(spans.items()):
        if "fillBuffer" in short and len(tv) > 8:
            print(f"  {short} grid {grid}, the twelve longest launches: " + " ".join("%.1f" % us for us in sorted((us for _, us in tv), reverse=True)[:12]))
    # the metrics fold's grid is capped, so both sizes of the leg launch the same one: its launches in start order, the smaller size first
    for (short, grid), tv in sorted(spans.items()):
        if short.startswith("k_metrics_fold") or short.startswith("k_conn_claim"):     # k_conn_claim: the tool's overflowed first attempts come first
            print(f"  {short} grid {grid}, launches in start order: " + " ".join("%.1f" % us for _, us in sorted(tv)))


if "--k8s-trace" in sys.argv[1:]:
    k8s_trace(sys.argv[sys.argv.index("--k8s-trace") + 1])
    sys.exit(0)


def read_stream_rate():
    """Bytes per second of a plain read of 1 GiB (four times the Infinity Cache), the yardstick of the metrics leg."""
    x = torch.zeros(1 << 27, dtype=torch.int64, device="cuda")
    _, dt = timed(lambda: x.sum())
    return x.numel() * 8 / dt


def metrics_leg(tab, k8s, d_ev, m, d_rows, d_net):
    L = nf._lib
    ns = L.DIM_SRC_K8S(0) | L.DIM_DST_K8S(0) | L.DIM_FLOW_LAYER | L.DIM_SRC_SUBNET_LABEL | L.DIM_DST_SUBNET_LABEL
    workload = 0
    for f in (3, 2, 0):                                               # owner name, type, namespace
        workload |= L.DIM_SRC_K8S(f) | L.DIM_DST_K8S(f)
    workload |= L.DIM_FLOW_DIRECTION
    caps = [1 << 16, 1 << 16]
    with tab.metrics_table(k8s, [ns, workload]) as met:
        while True:
            d_groups = [torch.empty(c * 64, dtype=torch.uint8, device="cuda") for c in caps]
            fold = lambda: tab.metrics_fold_device(met, d_ev.data_ptr(), m, d_rows.data_ptr(), d_net.data_ptr(), caps, [g.data_ptr() for g in d_groups])  # noqa: E731
            rc, counts = fold()
            if rc == nf.OK:
                break
            caps = [min(4 * c, L.MET_MAX_GROUPS) for c in caps]
        (rc, counts), dt = timed(fold)
        assert rc == nf.OK
        groups = [g[: c * 64].cpu().numpy().view(nf.METRIC_GROUP) for g, c in zip(d_groups, counts)]
        assert all(int(g["flows"].sum()) == m for g in groups)
    # a lane reads three 16-byte units of its record (protocol; bytes; packets and ethertype), its 8 bytes of Kubernetes rows, its 8
    # bytes of net row, two class words per grouping, and the two rows' flag words because a grouping selects the layer
    per_flow = 48 + 8 + 8 + 2 * 8 + 8
    rate = read_stream_rate()
    print(f"  metrics  {m} flows -> {counts[0]} + {counts[1]} groups (caps {caps[0]}, {caps[1]}) in {dt * 1e3:.3f} ms per call = {m / dt / 1e6:.1f} M flows/s; "
          f"{per_flow} B read per flow = {per_flow * m / dt / 1e9:.1f} GB/s per call, {per_flow * m / dt / rate:.3f} of the read-stream rate "
          f"measured here ({rate / 1e9:.0f} GB/s over 1 GiB)")


def conntrack_leg(tab, d_ev, m, tls, k8s, net, d_off):
    L = nf._lib
    cap = 1 << 18
    d_ids = torch.empty(m, dtype=torch.int64, device="cuda")
    while True:
        d_out = torch.empty(cap * 128, dtype=torch.uint8, device="cuda")
        fold = lambda: tab.conn_fold_device(d_ev.data_ptr(), m, NOW, MONO, d_ids.data_ptr(), cap, d_out.data_ptr())  # noqa: E731
        rc, n_conns, n_disc = fold()
        if rc == nf.OK:
            break
        assert cap < L.CONN_MAX_CONNS, "more connections than NFAGG_CONN_MAX_CONNS"
        cap = min(max(4 * cap, n_conns), L.CONN_MAX_CONNS)
    (rc, n_conns, n_disc), dt = timed(fold)
    assert rc == nf.OK
    parts = d_out[: n_conns * 128].cpu().numpy().view(nf.CONN_PARTIAL)
    assert int(parts["flows"].sum()) == m - n_disc and int((d_ids == 0).sum()) >= n_disc
    # k_conn_claim reads five 16-byte units of the record and writes the hash id, hashA and the slot; k_conn_finish reads the slot,
    # hashA, two units of the record again and, for a flow that is not its connection's first, that flow's hashA
    later = m - n_disc - n_conns
    read, wrote = 80 + 12 + 32 + 8 * later / m, 20
    slots = max(1024, 1 << (2 * min(cap, m) - 1).bit_length())
    print(f"  conntrack {m} flows -> {n_conns} connections, {n_disc} discarded (cap {cap}, {slots} slots = {slots * 128 >> 20} MiB zeroed per call) "
          f"in {dt * 1e3:.3f} ms per call = {m / dt / 1e6:.1f} M flows/s; {read:.0f} B read + {wrote} B written per flow by this tool's count = "
          f"{(read + wrote) * m / dt / 1e9:.1f} GB/s per call")
    del d_out
    # the flow logs: the _net line plus _HashId and _RecordType for the flows the stage tracks, no line for the others
    args = (d_ev.data_ptr(), m, tls, k8s, net, d_ids.data_ptr(), NOW, MONO, names, agent, 1_700_000_000)
    rc, need = tab.encode_flp_json_conn_device(*args, 0, 0, d_off.data_ptr())
    d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    (rc, wrote), dt = timed(lambda: tab.encode_flp_json_conn_device(*args, d_out.data_ptr(), need, d_off.data_ptr()))
    assert rc == nf.OK and wrote == need
    per_byte("_conn", m, dt, wrote)
    print(f"           flow logs: {m - n_disc} of {m} flows tracked, {wrote / max(m - n_disc, 1):.1f} B per line that is written")
    del d_out
    if LOKI:
        loki_leg(tab, d_ev, m, tls, k8s, net, d_ids, dt)
    # the conversation records at the leg's connection count: every connection's first flow is its carrier, the values are the partials'
    # sums with synthetic all-zero snapshots. The byte sums are masked to 40 bits so that no conversation is deferred (the synthetic
    # flows' byte counts are random 64-bit values): the leg times the encoder writing every line. The fields are the operator's usual
    # ones by name and width; `FlowDirection` is only a name here, a `first` column that reads the snapshot's Dscp (a conversation has
    # no FlowDirection of its own)
    fields = [dict(name="Bytes", operation="sum", splitAB=True), dict(name="Packets", operation="sum", splitAB=True),
              dict(name="numFlowLogs", operation="count"), dict(name="TimeFlowStart", operation="min", input="TimeFlowStartMs"),
              dict(name="TimeFlowEnd", operation="max", input="TimeFlowEndMs"), dict(name="FlowDirection", operation="first", input="Dscp"),
              dict(name="IfDirection", operation="first", input="IfDirections")]
    vals = np.zeros(n_conns, dtype=nf.CONN_VALUES)
    vals["hash_total"], vals["flows"], vals["bytes"], vals["packets"] = parts["hash_total"], parts["flows"], parts["bytes"] & ((1 << 40) - 1), parts["packets"]
    vals["start_ms_min"], vals["end_ms_max"], vals["is_first"] = parts["start_ms_min"], parts["end_ms_max"], 1
    vals["first"]["n_dirs"] = vals["last"]["n_dirs"] = 1
    d_vals = torch.from_numpy(vals.view(np.uint8).reshape(-1)).cuda()
    d_car = d_ev.view(torch.uint8)[: m * 144].view(m, 144)[torch.from_numpy(parts["first_idx"].astype(np.int64)).cuda()].contiguous()
    with tab.conn_layout(fields) as lay:
        cargs = (d_car.data_ptr(), d_vals.data_ptr(), n_conns, lay, k8s, net)
        rc, need, n_def = tab.encode_conn_json_device(*cargs, 0, 0, d_off.data_ptr())
        d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
        (rc, wrote, n_def), dt = timed(lambda: tab.encode_conn_json_device(*cargs, d_out.data_ptr(), need, d_off.data_ptr()))
        assert rc == nf.OK and wrote == need
        per_byte("conv", n_conns, dt, wrote)
        print(f"           conversation records: {lay.n_columns} columns, longest possible line {lay.max_line} B, {n_def} deferred")


def timebased_leg(tab, k8s, d_ev, m, d_rows, n_distinct):
    L = nf._lib
    second, window = 10**9, 12
    recs = d_ev.view(torch.uint8)[: m * 144].view(m, 144)
    keep = recs[:, 56:64].contiguous().view(torch.int64).reshape(-1) != 0          # a flow without Bytes has no operation key: dropped first
    kept = int(keep.sum())
    rows = d_rows
    if kept != m:
        recs, rows = recs[keep].contiguous(), d_rows[keep].contiguous()
    specs = [dict(index_keys=keys, operation=L.TB_OP_SUM, value=L.MET_VALUE_BYTES, top_k=10, interval_ns=(window - 1) * second)
             for keys in (["SrcAddr"], ["SrcK8S_Namespace", "DstK8S_Namespace"])]
    max_keys = min(L.TB_MAX_KEYS, max(1024, n_distinct))
    d_outs = [torch.empty(10 * 16, dtype=torch.uint8, device="cuda") for _ in specs]
    ptrs = [o.data_ptr() for o in d_outs]
    with tab.timebased_rules(specs, k8s, None, max_keys) as tb:
        now = [0]

        def call():
            now[0] += second
            return tab.timebased_extract_device(tb, recs.data_ptr(), kept, now[0], rows.data_ptr(), 0, [10, 10], ptrs)
        for _ in range(window):                                                    # fill the window: every later call merges 12 slices per rule
            rc, counts, missing = call()
            assert (rc, missing) == (nf.OK, 0), (rc, missing)
        (rc, counts, missing), dt = timed(call)
        st = tb.stats()
        assert rc == nf.OK and counts == [min(10, st.keys[0]), min(10, st.keys[1])], (rc, counts, missing, st.failed)   # at the larger size no flow has both namespaces
        (rc, counts), dt_eval = timed(lambda: tab.timebased_results_device(tb, [10, 10], ptrs))
        assert rc == nf.OK
        st = tb.stats()
        top = [o.cpu().numpy().view(nf.TB_RESULT) for o in d_outs]
        assert all((np.diff(t["value"]) <= 0).all() for t in top) and st.slices[0] == window and st.slices[1] in (0, window)
    print(f"  timebased {kept} of {m} flows (the others have no Bytes) -> {st.keys[0]} addresses in {st.slots[0]} slots, {st.keys[1]} namespace pairs; "
          f"{window} slices in the window, {st.bytes_held >> 20} MiB held; {dt * 1e3:.3f} ms per call = {kept / dt / 1e6:.1f} M flows/s; "
          f"the evaluation alone (2 rules x {window} slices, value, select, sort): {dt_eval * 1e3:.3f} ms; "
          f"{int(top[0]['flags'].sum())} + {int(top[1]['flags'].sum())} of the {counts[0]} + {counts[1]} results inexact (totals of 2^53 or more)")


def loki_leg(tab, d_ev, m, tls, k8s, net, d_ids, dt_conn):
    import ctypes as C
    L = nf._lib
    o, keep = nf.flp_options(NOW, MONO, names, agent, 1_700_000_000, b"unknown")
    labels = ["SrcK8S_Namespace", "SrcK8S_OwnerName", "SrcK8S_OwnerType", "DstK8S_Namespace", "DstK8S_OwnerName", "DstK8S_OwnerType", "K8S_FlowLayer", "FlowDirection",
              "_RecordType"]
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for batch_size in (100 * 1024, 10 << 20):
        w = nf.WriteLoki(dict(labels=labels, timestampLabel="TimeFlowEndMs", timestampScale="1ms", batchSize=batch_size, staticLabels={"app": "netobserv-flowcollector"}))
        with tab.loki_table(w, k8s, net) as lt:
            cap_s, cap_g = min(m, L.LOKI_MAX_STREAMS), m
            d_streams = torch.empty(cap_s * 20 + 16, dtype=torch.uint8, device="cuda")
            d_groups = torch.empty(cap_g * 24 + 16, dtype=torch.uint8, device="cuda")
            counts = L.LokiCounts()
            plan = lambda: L.lib.nfagg_loki_plan_device(tab._h, ptr(d_ev), m, None, None, None, tls._t, k8s._t, net._t, ptr(d_ids), C.byref(o), lt._t, NOW, ptr(d_streams),  # noqa: E731
                                                        cap_s, ptr(d_groups), cap_g, None, C.byref(counts))
            rc, dt_plan = timed(plan)
            if rc != L.OK:
                print(f"  _loki    batch size {batch_size}: the plan is refused ({(L.lib.nfagg_last_error(tab._h) or b'').decode()})")
                continue
            streams = d_streams[: counts.n_streams * 20].cpu().numpy().view(nf.LOKI_STREAM)
            t0 = time.perf_counter()
            texts = lt.labels_of(streams)
            dt_labels = time.perf_counter() - t0
            blob = b"".join(texts)
            off = np.zeros(len(texts) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(t) for t in texts], dtype=np.uint64)
            d_boff = torch.empty(counts.n_batches + 1, dtype=torch.int64, device="cuda")
            d_bent = torch.empty(counts.n_batches + 1, dtype=torch.int32, device="cuda")
            need = C.c_size_t(0)
            rc = L.lib.nfagg_loki_write_device(tab._h, blob, off.ctypes.data_as(C.c_void_p), None, 0, ptr(d_boff), ptr(d_bent), C.byref(need))
            total = need.value
            d_out = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
            rc, dt_write = timed(lambda: L.lib.nfagg_loki_write_device(tab._h, blob, off.ctypes.data_as(C.c_void_p), ptr(d_out), total, ptr(d_boff), ptr(d_bent), C.byref(need)))
            assert rc == L.OK and need.value == total and int(d_boff[counts.n_batches]) == total
            whole = dt_plan + dt_labels + dt_write
            print(f"  _loki    batch size {batch_size}: {m} flows -> {counts.n_streams} streams, {counts.n_groups} groups, {counts.n_batches} batches, {counts.n_deferred} deferred, "
                  f"{total} bytes; plan {dt_plan * 1e3:.3f} ms, label texts on the host {dt_labels * 1e3:.3f} ms ({len(blob)} B), write {dt_write * 1e3:.3f} ms, "
                  f"whole call {whole * 1e3:.3f} ms = {m / whole / 1e6:.2f} M flows/s, {dt_write / max(total, 1) * 1e12:.3f} ps per output byte of the write; "
                  f"plan + write = {(dt_plan + dt_write) / dt_conn:.2f} of the _conn call of this run ({dt_conn * 1e3:.3f} ms)")
            del d_out, d_streams, d_groups


def metrics_content_leg(tab, k8s, d_ev, m, d_rows, d_net):
    L = nf._lib
    ns = L.DIM_SRC_K8S(0) | L.DIM_DST_K8S(0)
    rtt = [int(b * 1e9) for b in (.005, .01, .025, .05, .1, .25, .5, 1, 2.5, 5)]
    dns = [int(b * 1000) for b in (.005, .01, .025, .05, .1, .25, .5, 1, 2.5, 5, 10)]
    specs = [dict(dims=ns, value=(L.MET_VALUE_RTT_NS,), hist=1, bounds=rtt),
             dict(dims=ns, xdims=L.XDIM_DNS_RCODE, value=(L.MET_VALUE_DNS_LATENCY_MS,), hist=1, bounds=dns),
             dict(dims=ns, xdims=L.XDIM_DROP_CAUSE | L.XDIM_DROP_STATE, value=(L.MET_VALUE_DROP_BYTES, L.MET_VALUE_DROP_PACKETS))]
    d_present, d_parts = device_parts(m)
    feat = (d_present.data_ptr(), {k: d_parts[k].data_ptr() for k in ("additional", "dns", "drops")})
    caps = [1 << 16] * 3
    with tab.metrics_table_specs(k8s, specs) as met:
        while True:
            d_groups = [torch.empty(c * 128, dtype=torch.uint8, device="cuda") for c in caps]
            fold = lambda: tab.metrics_fold_content_device(met, d_ev.data_ptr(), m, d_rows.data_ptr(), d_net.data_ptr(), caps,  # noqa: E731
                                                           [g.data_ptr() for g in d_groups], feat)
            rc, counts = fold()
            if rc == nf.OK:
                break
            caps = [min(4 * c, L.MET_MAX_GROUPS) if n > c else c for n, c in zip(counts, caps)]
        (rc, counts), dt = timed(fold)
        assert rc == nf.OK
        groups = [g[: c * 128].cpu().numpy().view(nf.METRIC_GROUP_CONTENT) for g, c in zip(d_groups, counts)]
        assert all(int(g["flows"].sum()) == m for g in groups)
    with_parts = int((d_present != 0).sum())
    # a lane reads the three 16-byte units of its record, its 8 bytes of Kubernetes rows, its 8 bytes of net row (unused by these
    # groupings, loaded all the same), two class words per grouping, its present byte and, with the parts, one 16-byte unit of each of three
    per_flow = 48 + 8 + 8 + 3 * 8 + 1 + 48 * with_parts / m
    rate = read_stream_rate()
    print(f"  metrics content ({os.path.basename(L.LIB_PATH)}) {m} flows, parts on {with_parts} -> {' + '.join(str(c) for c in counts)} groups "
          f"(caps {', '.join(str(c) for c in caps)}) in {dt * 1e3:.3f} ms per call = {m / dt / 1e6:.1f} M flows/s; "
          f"{per_flow:.0f} B read per flow = {per_flow * m / dt / 1e9:.1f} GB/s per call, {per_flow * m / dt / rate:.3f} of the read-stream rate "
          f"measured here ({rate / 1e9:.0f} GB/s over 1 GiB)")


def filter_leg(tab, d_ev, m, tls, k8s, net, d_rows, d_net, d_off, dt_net_join, dt_net_encode):
    recs = d_ev[: m * 144].cpu().numpy().view(nf.FLOW_RECORD)
    p, q = int(np.quantile(recs["id"]["src_port"], 0.5)), int(np.quantile(recs["id"]["dst_port"], 0.3))
    query = "(SrcPort < %d or DstPort < %d) and with(Bytes)" % (p, q)
    del recs
    rate = read_stream_rate()
    d_keep, d_rule = torch.empty(m, dtype=torch.uint8, device="cuda"), torch.empty(m, dtype=torch.uint8, device="cuda")
    d_idx, d_out = torch.empty(m, dtype=torch.int32, device="cuda"), torch.empty(m * 144 + 16, dtype=torch.uint8, device="cuda")
    print(f"  filter   keep_entry_query: {query}; the unfiltered _net call {dt_net_encode * 1e3:.3f} ms, the net join {dt_net_join * 1e3:.3f} ms, "
          f"read stream {rate / 1e9:.0f} GB/s over 1 GiB")
    for sampling in (0, 10):
        cfg = dict(samplingField="Sampling", rules=[dict(type="keep_entry_query", keepEntryQuery=query, keepEntrySampling=sampling)])
        with tab.filter(nf.TransformFilter(cfg)) as flt:
            apply = lambda: tab.filter_apply_device(flt, d_ev.data_ptr(), m, d_rows.data_ptr(), d_net.data_ptr(), None, NOW, MONO, 1, 0, d_keep.data_ptr(),  # noqa: E731
                                                    d_rule.data_ptr(), d_idx.data_ptr(), d_out.data_ptr(), m)
            (rc, kept, n_def), dt_apply = timed(apply)
            (_, kept0, _), dt_eval = timed(lambda: tab.filter_apply_device(flt, d_ev.data_ptr(), m, 0, 0, None, NOW, MONO, 1, 0, d_keep.data_ptr(), d_rule.data_ptr()))
            assert rc == nf.OK and kept0 == kept and int((d_keep != 0).sum()) == kept
            d_rows2, d_net2 = torch.empty((max(kept, 1), 2), dtype=torch.int32, device="cuda"), torch.empty((max(kept, 1), 2), dtype=torch.int32, device="cuda")
            _, dt_gather = timed(lambda: (tab.gather_device(d_rows.data_ptr(), m, 8, d_idx.data_ptr(), kept, d_rows2.data_ptr()),
                                          tab.gather_device(d_net.data_ptr(), m, 8, d_idx.data_ptr(), kept, d_net2.data_ptr())))
            rc, need = tab.encode_flp_json_net_device(d_out.data_ptr(), kept, tls, k8s, net, NOW, MONO, names, agent, 1_700_000_000, 0, 0, d_off.data_ptr())
            d_lines = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
            (rc, wrote), dt_enc = timed(lambda: tab.encode_flp_json_net_device(d_out.data_ptr(), kept, tls, k8s, net, NOW, MONO, names, agent, 1_700_000_000,
                                                                              d_lines.data_ptr(), need, d_off.data_ptr()))
            assert rc == nf.OK and wrote == need
            del d_lines
        # eval: a lane reads its record and writes keep, rule, the sampling and its scan offset; compact: per flow the scan offsets of a
        # flow and its successor, per kept flow the record read and written, the sampling read, the index written
        ev_bytes, co_bytes = m * (144 + 1 + 1 + 4 + 4), m * 8 + kept * (2 * 144 + 4 + 4)
        dt_compact = max(dt_apply - dt_eval, 1e-9)
        print(f"  filter   sampling {sampling:2d}: {kept} of {m} flows kept ({kept / m:.3f}), {n_def} deferred; apply {dt_apply * 1e3:.3f} ms per call = "
              f"{m / dt_apply / 1e6:.1f} M flows/s ({dt_apply / dt_net_join:.2f} x the net join); without the compaction {dt_eval * 1e3:.3f} ms = "
              f"{ev_bytes / dt_eval / 1e9:.1f} GB/s, {ev_bytes / dt_eval / rate:.3f} of the read stream; the compaction's share {dt_compact * 1e3:.3f} ms = "
              f"{co_bytes / dt_compact / 1e9:.1f} GB/s, {co_bytes / dt_compact / rate:.3f} of the read stream")
        print(f"           gather of both row arrays {dt_gather * 1e3:.3f} ms; _net on the kept flows {dt_enc * 1e3:.3f} ms for {wrote} bytes "
              f"({dt_enc / dt_net_encode:.3f} of the unfiltered call); apply + gather + encode = {(dt_apply + dt_gather + dt_enc) / dt_net_encode:.3f} of it")


def ipfix_leg(tab, d_ev, m, entries, d_rows, d_off, dt_net_encode):
    """nfagg_flp_ipfix_write_device on the leg's records and rows, and the agent's own IPFIX encoder beside it."""
    import ctypes as C
    from netobserv_ebpf_agent_amd.flp_ipfix import flp_ipfix_options
    L = nf._lib
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with tab.flp_ipfix_strings(entries) as strings, tab.flp_ipfix_writer() as state:
        o, keep = flp_ipfix_options(NOW, MONO, names, 1_700_000_000, 0, 2, 65535)
        d_status = torch.empty(m + 16, dtype=torch.uint8, device="cuda")
        need, sent = C.c_size_t(0), C.c_size_t(0)
        args = (tab._h, state._t, ptr(d_ev), m, None, ptr(d_rows), strings._t, C.byref(o))
        for _ in range(2):        # the first call starts from NewWriteIpfix's state, every later one from the state a whole pass left: sized again
            rc = L.lib.nfagg_flp_ipfix_write_device(*args, None, 0, ptr(d_off), ptr(d_status), C.byref(sent), C.byref(need))
            assert rc == L.TRUNCATED, L.lib.nfagg_last_error(tab._h)
            total = need.value
            d_out = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
            rc = L.lib.nfagg_flp_ipfix_write_device(*args, ptr(d_out), total, ptr(d_off), ptr(d_status), C.byref(sent), C.byref(need))
            assert rc == L.OK and need.value == total, L.lib.nfagg_last_error(tab._h)
        rc, dt = timed(lambda: L.lib.nfagg_flp_ipfix_write_device(*args, ptr(d_out), total, ptr(d_off), ptr(d_status), C.byref(sent), C.byref(need)))
        assert rc == L.OK and need.value == total, L.lib.nfagg_last_error(tab._h)
        per_byte("_wipfix", m, dt, need.value)
        # per flow: the record, 4 B of meta written and read twice, 64 B of sources written and read twice (rewritten where a source lay
        # before the block), 32 B of interface rows written and read, 8 B of rows read three times, two 4-byte scan words written and
        # read, the 8-byte offset and the status byte written; the strings and the source flows' records on top are not counted
        moved = m * (2 * 144 + 3 * 4 + 3 * 64 + 2 * 32 + 3 * 8 + 4 * 4 + 8 + 1) + need.value
        print(f"           {sent.value} of {m} flows sent, {m - sent.value} failed; {moved / dt / 1e9:.1f} GB/s by this tool's count of a flow's own bytes; "
              f"the _net call of this run: {dt_net_encode * 1e3:.3f} ms")
        del d_out
    rc, need2 = tab.encode_ipfix_device(d_ev.data_ptr(), m, NOW, MONO, names, 1_700_000_000, 0, 0, 0, d_off.data_ptr())
    d_out = torch.empty(need2 + 16, dtype=torch.uint8, device="cuda")
    (rc, wrote), dt2 = timed(lambda: tab.encode_ipfix_device(d_ev.data_ptr(), m, NOW, MONO, names, 1_700_000_000, 0, d_out.data_ptr(), need2, d_off.data_ptr()))
    assert rc == nf.OK and wrote == need2
    per_byte("_ipfix", m, dt2, wrote)


def per_byte(what, m, dt, wrote):
    print(f"  {what:8s} {m} flows -> {wrote} bytes ({wrote / m:.1f} B/line) in {dt * 1e3:.3f} ms per call = {m / dt / 1e6:.1f} M flows/s, "
          f"{dt / wrote * 1e12:.3f} ps per output byte")


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


for flows in ((FLOWS,) if FLOWS else (10_000_000,) if (CONTENT or TLS) and not K8S else (1_000_000, 10_000_000)):
    if K8S:
        torch.cuda.empty_cache()
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
        if K8S:
            entries, n_distinct, n_ip = k8s_entries(d_ev, m)
            d_off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
            d_rows = torch.empty((m, 2), dtype=torch.int32, device="cuda")
            with tab.tls_names() as tls, tab.k8s_table(entries, (["openshift", "kube-"], [("ns-1", "pod-1")])) as k8s:
                rc, need = tab.encode_flp_json_tls_device(d_ev.data_ptr(), m, tls, NOW, MONO, names, agent, 1_700_000_000, 0, 0, d_off.data_ptr())
                d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
                (rc, wrote), dt = timed(lambda: tab.encode_flp_json_tls_device(d_ev.data_ptr(), m, tls, NOW, MONO, names, agent, 1_700_000_000,
                                                                              d_out.data_ptr(), need, d_off.data_ptr()))
                assert rc == nf.OK and wrote == need
                per_byte("_tls", m, dt, wrote)
                del d_out
                _, dt_res = timed(lambda: tab.k8s_resolve_device(k8s, d_ev.data_ptr(), m, d_rows.data_ptr()))
                hits = int((d_rows != -1).sum())
                rc, need = tab.encode_flp_json_k8s_device(d_ev.data_ptr(), m, tls, k8s, NOW, MONO, names, agent, 1_700_000_000, 0, 0, d_off.data_ptr())
                d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
                (rc, wrote), dt = timed(lambda: tab.encode_flp_json_k8s_device(d_ev.data_ptr(), m, tls, k8s, NOW, MONO, names, agent, 1_700_000_000,
                                                                              d_out.data_ptr(), need, d_off.data_ptr()))
                assert rc == nf.OK and wrote == need
                per_byte("_k8s", m, dt, wrote)
                print(f"           table: {len(entries)} rows, {min(K8S_ROWS, (n_distinct + 1) // 2)} of them among the {n_distinct} distinct addresses of {n_ip} IP flows; "
                      f"{hits} of {2 * m} endpoints resolved; the hash join alone: {dt_res * 1e3:.3f} ms per call")
                del d_out
                if NET:
                    flags = nf._lib.NET_REINTERPRET_DIRECTION | nf._lib.NET_SUBNET_LABELS | nf._lib.NET_DECODE_TCP_FLAGS
                    d_net = torch.empty((m, 2), dtype=torch.int32, device="cuda")
                    with tab.net_table(flags, NET_CATEGORIES) as net:
                        tab.k8s_resolve_device(k8s, d_ev.data_ptr(), m, d_rows.data_ptr())
                        _, dt_net = timed(lambda: tab.net_resolve_device(net, d_ev.data_ptr(), m, d_net.data_ptr(), k8s, d_rows.data_ptr(), agent))
                        got = d_net.cpu().numpy().view(nf.NET_ROW).reshape(-1)
                        rc, need = tab.encode_flp_json_net_device(d_ev.data_ptr(), m, tls, k8s, net, NOW, MONO, names, agent, 1_700_000_000, 0, 0,
                                                                  d_off.data_ptr())
                        d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
                        (rc, wrote), dt = timed(lambda: tab.encode_flp_json_net_device(d_ev.data_ptr(), m, tls, k8s, net, NOW, MONO, names, agent,
                                                                                      1_700_000_000, d_out.data_ptr(), need, d_off.data_ptr()))
                        assert rc == nf.OK and wrote == need
                        per_byte("_net", m, dt, wrote)
                        print(f"           rules: all three, {net.n_cidrs} CIDRs in {net.n_labels} categories; "
                              f"{int((got['src_label'] != nf._lib.NET_NO_LABEL).sum() + (got['dst_label'] != nf._lib.NET_NO_LABEL).sum())} of {2 * m} endpoints labelled, "
                              f"{int((got['direction'] != nf._lib.NET_NO_DIRECTION).sum())} of {m} flows with a direction; the join alone: {dt_net * 1e3:.3f} ms per call")
                        del d_out
                        if IPFIX:
                            tab.k8s_resolve_device(k8s, d_ev.data_ptr(), m, d_rows.data_ptr())
                            ipfix_leg(tab, d_ev, m, entries, d_rows, d_off, dt)
                        if FILTER:
                            filter_leg(tab, d_ev, m, tls, k8s, net, d_rows, d_net, d_off, dt_net, dt)
                        if METRICS:
                            metrics_leg(tab, k8s, d_ev, m, d_rows, d_net)
                            if CONNTRACK:
                                conntrack_leg(tab, d_ev, m, tls, k8s, net, d_off)
                                if TIMEBASED:
                                    tab.k8s_resolve_device(k8s, d_ev.data_ptr(), m, d_rows.data_ptr())
                                    timebased_leg(tab, k8s, d_ev, m, d_rows, n_distinct)
                            if CONTENT:
                                metrics_content_leg(tab, k8s, d_ev, m, d_rows, d_net)
                    del d_net
            del d_ev, d_off, d_rows
            continue
        # direct-FLP JSON
        d_off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
        d_def = torch.empty(m, dtype=torch.uint8, device="cuda")
        rc, need, n_def = tab.encode_flp_json_device(d_ev.data_ptr(), m, NOW, MONO, names, agent, 1_700_000_000, 0, 0, d_off.data_ptr())
        d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
        (rc, wrote, n_def), dt = timed(lambda: tab.encode_flp_json_device(d_ev.data_ptr(), m, NOW, MONO, names, agent, 1_700_000_000,
                                                                          d_out.data_ptr(), need, d_off.data_ptr(), d_def.data_ptr()))
        assert rc == nf.OK and wrote == need and n_def == 0
        if TLS:
            per_byte("no TLS", m, dt, wrote)
            print(f"           {dt / m * 1e9:.3f} ns per flow")
            del d_out
            n_on = set_tls_fields(d_ev, m)
            with tab.tls_names() as tls:
                rc, need = tab.encode_flp_json_tls_device(d_ev.data_ptr(), m, tls, NOW, MONO, names, agent, 1_700_000_000, 0, 0, d_off.data_ptr())
                d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
                (rc, wrote), dt = timed(lambda: tab.encode_flp_json_tls_device(d_ev.data_ptr(), m, tls, NOW, MONO, names, agent, 1_700_000_000,
                                                                              d_out.data_ptr(), need, d_off.data_ptr()))
            assert rc == nf.OK and wrote == need
            per_byte("TLS", m, dt, wrote)
            print(f"           {dt / m * 1e9:.3f} ns per flow; TLS fields on {n_on} of {m} flows")
            continue
        if CONTENT:
            per_byte("plain", m, dt, wrote)
            del d_out
            d_present, d_parts = device_parts(m)
            feat = (d_present.data_ptr(), {k: v.data_ptr() for k, v in d_parts.items()})
            rc, need, n_def = tab.encode_flp_json_content_device(d_ev.data_ptr(), m, *feat, NOW, MONO, names, agent, 1_700_000_000, 0, 0,
                                                                 d_off.data_ptr())
            d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
            (rc, wrote, n_def), dt = timed(lambda: tab.encode_flp_json_content_device(
                d_ev.data_ptr(), m, *feat, NOW, MONO, names, agent, 1_700_000_000, d_out.data_ptr(), need, d_off.data_ptr(), d_def.data_ptr()))
            assert rc == nf.OK and wrote == need and n_def == 0
            per_byte("content", m, dt, wrote)
            print(f"  parts on {int((d_present != 0).sum())} of {m} flows")
            continue
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
