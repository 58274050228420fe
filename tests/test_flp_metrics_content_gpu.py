"""Content flow metrics on the GPU (nfagg_metrics_fold_content, k_metrics_fold_content of csrc/nfagg_metrics.hip) through the C
ABI, host and device entry points: PromMetrics.observe on merged MapTracer flows against the per-flow restatement of
tests/flp_metrics_content_ref.py; the fold against a numpy group-by with the four extra key columns and the bucket; a plain table
against nfagg_metrics_fold; bucket edges; the presence rules and the arithmetic of the values; one hot (group, bucket); more groups
than any LDS table holds, truncation and exact caps; eight specs in one call; keys crafted onto one slot that differ in their third
word alone. Records, informer answers, layer rule and subnet categories are those of tests/test_flp_metrics_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_content_ref as C  # noqa: E402
import flp_json_k8s_ref as K  # noqa: E402
import flp_json_net_ref as R  # noqa: E402
import flp_metrics_content_ref as H  # noqa: E402
import flp_metrics_ref as M  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_flp_json_net_cpu as NC  # noqa: E402
import test_flp_json_net_gpu as NG  # noqa: E402
import test_flp_metrics_gpu as MG  # noqa: E402
import test_netev_gpu as E  # noqa: E402
from flp_json_ref import record_to_map  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, NOW, MONO, RECEIVED = G.NAMES, G.NOW, G.MONO, G.RECEIVED
LAYER, CATEGORIES, REPORTER, ALL = MG.LAYER, MG.CATEGORIES, MG.REPORTER, MG.ALL
I64_MIN, I64_MAX = -2**63, 2**63 - 1
KEY = ["src_class", "dst_class", "src_label", "dst_label", "direction", "layer", "proto", "is_ip", "drop_cause", "drop_state", "dns_rcode", "ipsec_status", "bucket"]
SUMS = ["flows", "bytes", "packets", "flows_with_bytes", "flows_with_packets"]
NS = ["SrcK8S_Namespace", "DstK8S_Namespace"]

# the operator's shapes: RTT and DNS-latency histograms, the drop counters by state and cause, the IPsec counters; a histogram
# over Bytes; a counter that shares the RTT histogram's grouping and slot; DnsId as a filter; DefBuckets throughout
ITEMS = [
    dict(name="namespace_rtt_seconds", type="histogram", valueKey="TimeFlowRttNs", valueScale=1e9, labels=NS),
    dict(name="namespace_dns_latency_seconds", type="histogram", valueKey="DnsLatencyMs", valueScale=1000, labels=NS + ["DnsFlagsResponseCode"],
         filters=[dict(key="DnsId", type="presence")]),
    dict(name="namespace_drop_bytes_total", type="counter", valueKey="PktDropBytes", labels=NS + ["PktDropLatestState", "PktDropLatestDropCause"]),
    dict(name="namespace_drop_packets_total", type="counter", valueKey="PktDropPackets", labels=NS + ["PktDropLatestState", "PktDropLatestDropCause"]),
    dict(name="node_ipsec_flows_total", type="counter", labels=["SrcK8S_HostName", "IPSecStatus"], filters=[dict(key="IPSecStatus", type="presence")]),
    dict(name="flow_kbytes", type="histogram", valueKey="Bytes", valueScale=1000, labels=["K8S_FlowLayer", "FlowDirection"]),
    dict(name="namespace_rtt_ns_total", type="counter", valueKey="TimeFlowRttNs", labels=NS),
    dict(name="namespace_flows_total", type="counter", labels=NS, remap={"SrcK8S_Namespace": "src"}),
    dict(name="undns_bytes_total", type="counter", valueKey="Bytes", valueScale=1, labels=["DstSubnetLabel"], filters=[dict(key="DnsId", type="absence")]),
]
SCALE = {"netobserv_" + it["name"]: it.get("valueScale", 0) for it in ITEMS}


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


def bounded(recs, present, parts, rng):
    """The merged flows with their values bounded and not negative: the device's sums are 64-bit integers (modulo 2^64,
    include/nfagg.h) and the reference's are floats, so a test of their agreement keeps every sum inside int64. The RTT and
    the latency are spread over every DefBucket of the items' scales, a third of the ids are 0 (no DNS keys), a third of the causes
    0 (no drop keys) or a known one. make_maps leaves a part on a tenth to a quarter of the flows: each of the three parts the
    metrics read is put on about half of them here, its other fields as the merge left them (zero where it had no part)."""
    n = len(recs)
    recs, parts = recs.copy(), {k: v.copy() for k, v in parts.items()}
    present = (present & ~np.uint8(7)) | rng.integers(0, 8, n).astype(np.uint8)
    recs["metrics"]["bytes"] = np.where(rng.integers(0, 4, n) == 0, 0, 10 ** rng.integers(0, 7, n) * rng.integers(1, 10, n)).astype(np.uint64)
    recs["metrics"]["bytes"][::7] = 2**52
    a, d, p = parts["additional"], parts["dns"], parts["drops"]
    a["flow_rtt"] = np.where(rng.integers(0, 3, n) == 0, 0, 10 ** rng.integers(5, 11, n) * rng.integers(1, 10, n)).astype(np.uint64)
    a["flow_rtt"][::9] = 2**55
    a["ipsec_encrypted_ret"] = np.where(rng.integers(0, 3, n) == 0, rng.integers(-200, 200, n), 0)
    a["ipsec_encrypted"] = rng.integers(0, 2, n)
    d["latency"] = (10 ** rng.integers(5, 11, n) * rng.integers(0, 10, n)).astype(np.uint64)
    d["id"] = np.where(rng.integers(0, 3, n) == 0, 0, d["id"] | 1)
    d["flags"] = np.where(rng.integers(0, 2, n) == 0, d["flags"], d["flags"] & 0xFFF0 | rng.integers(0, 4, n).astype(np.uint16))
    p["latest_drop_cause"] = np.array([0, 2, 5, 77, (3 << 16) + 3, (1 << 24) + 4, 9999], dtype=np.uint32)[rng.integers(0, 7, n)]
    p["latest_state"] = np.where(rng.integers(0, 2, n) == 0, p["latest_state"], rng.integers(0, 13, n)).astype(np.uint8)
    return recs, present, {**parts, "additional": a, "dns": d, "drops": p}


@pytest.fixture(scope="module")
def world(nf, O, tab):
    """About 300 merged MapTracer flows (test_map_merge.make_maps: some exist in a feature map only; each part on about half of
    them), the informer answers for half of their addresses, and per flow the restatement's enriched map."""
    from test_map_merge import make_maps
    main_ids, main_vals, feats = make_maps(O, seed=11, n_pop=400, n_main=300, n_feat=250, n_cpu=4)
    main_vals["eth_protocol"] = 0x86DD
    recs, present, parts, _ = tab.map_merge(main_ids, main_vals, feats, 4)
    recs, present, parts = bounded(recs, present, parts, np.random.default_rng(3))
    entries = MG.KG.entries_for(recs)
    table, cats, names = K.table_of(entries), R.parse_subnets(CATEGORIES), G.rows(NAMES)
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 144)
    maps, memo = [], {}
    for i in range(len(raw)):
        m = record_to_map(raw[i].tobytes(), NOW, MONO, names, REPORTER, RECEIVED, b"unknown", memo)
        maps.append(R.apply_rules(C.add_content(m, C.flow_parts(present, parts, i)), table, LAYER, ALL, cats))
    print("flows:", len(recs), "with additional / dns / drops:", [int(np.sum(present & bit != 0)) for bit in (1, 2, 4)])
    assert 250 < len(recs) < 450 and all(0.4 < np.mean(present & bit != 0) < 0.6 for bit in (1, 2, 4))
    return recs, present, parts, entries, maps


# ---- 1. parity with the per-flow restatement
def check_metrics(p, maps, calls=1):
    """Counters by test_flp_metrics_gpu.check_counters' rule; a histogram's buckets and count exactly, its sum one rounding of the
    exact integer sum per call and within n roundings of the restatement's running float."""
    counters = [it for it in ITEMS if it["type"] == "counter"]
    hist_items = [it for it in ITEMS if it["type"] == "histogram"]
    ref_c, ref_h = M.Counters(counters, prefix="netobserv_"), H.Histograms(hist_items, prefix="netobserv_")
    for m in maps:
        ref_c.encode(m)
        ref_h.encode(m)
    exact = H.exact_sums(maps, ITEMS, "netobserv_")
    once = lambda key: float(exact[key]) / SCALE[key[0]] if SCALE[key[0]] else float(exact[key])  # noqa: E731
    assert set(p.values) == set(ref_c.values) and set(p.histograms) == set(ref_h.values)
    for key, v in ref_c.values.items():
        assert p.values[key] == calls * once(key), key
        assert abs(p.values[key] - calls * v) <= len(maps) * 2.0**-52 * abs(calls * v), key
    for key, h in ref_h.values.items():
        got = p.histograms[key]
        print(key[0], dict(key[1]), got["buckets"], got["count"], got["sum"], h["sum"])
        assert got["buckets"] == [calls * b for b in h["buckets"]] and got["count"] == calls * h["count"], key
        assert got["sum"] == calls * once(key), key
        assert abs(got["sum"] - calls * h["sum"]) <= len(maps) * 2.0**-52 * abs(calls * h["sum"]), key
    return ref_c.values, ref_h.values


def test_prom_metrics_against_the_restatement(nf, tab, world):
    recs, present, parts, entries, maps = world
    p = nf.PromMetrics(ITEMS, prefix="netobserv_")
    assert len(p.groupings) == 6
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, ALL, tab) as net:
        p.observe(tab, recs, k8s, net, REPORTER, features=(present, parts))
        ref_c, ref_h = check_metrics(p, maps)
        p.observe(tab, recs, k8s, net, REPORTER, features=dict(parts, present=present))       # a second eviction doubles everything
        check_metrics(p, maps, calls=2)
        q = nf.PromMetrics(ITEMS, prefix="netobserv_")                                         # no parts: the feature keys exist for no flow
        q.observe(tab, recs, k8s, net, REPORTER)
    for name in ("namespace_rtt_seconds", "namespace_dns_latency_seconds", "flow_kbytes"):         # every histogram spreads over its buckets
        mine = [h for (n, _), h in ref_h.items() if n == "netobserv_" + name]
        assert len(mine) >= 2 and sum(1 for k in range(12) if any(h["buckets"][k] for h in mine)) >= 6, name
    assert any(h["sum"] * SCALE[n] > 2.0**53 for (n, _), h in ref_h.items() if n == "netobserv_namespace_rtt_seconds")
    causes = {dict(l)["PktDropLatestDropCause"] for n, l in ref_c if n == "netobserv_namespace_drop_bytes_total"}
    assert {b"SKB_DROP_REASON_NOT_SPECIFIED", b"OVS_DROP_EXPLICIT", b"NetworkEvent_NetworkPolicy", b"SKB_DROP_UNKNOWN_CAUSE"} <= causes
    assert {dict(l)["IPSecStatus"] for n, l in ref_c if n == "netobserv_node_ipsec_flows_total"} == {b"success", b"error"}
    assert {n for n, _ in q.values} == {"netobserv_namespace_flows_total", "netobserv_undns_bytes_total"}
    assert {n for n, _ in q.histograms} == {"netobserv_flow_kbytes"}


def test_the_map_tracer_hands_its_features_to_the_metrics(nf, O, tab, world):
    from test_map_merge import make_maps
    _, _, _, entries, _ = world
    main_ids, main_vals, feats = make_maps(O, seed=11, n_pop=400, n_main=300, n_feat=250, n_cpu=4)
    main_vals["eth_protocol"] = 0x86DD
    mrecs, present, parts, _ = tab.map_merge(main_ids, main_vals, feats, 4)
    items = [it for it in ITEMS if it["name"] in ("namespace_dns_latency_seconds", "namespace_drop_packets_total", "node_ipsec_flows_total", "namespace_flows_total")]
    with tab.tls_names() as tls, tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, ALL, tab) as net:
        mt = nf.MapTracer(nf.GPUMapFetcher(tab, lambda: (main_ids, main_vals, feats, 4)), 0, 0, clock=lambda: NOW, mono_clock=lambda: MONO)
        traced, direct = nf.PromMetrics(items), nf.PromMetrics(items)
        lines = mt.evictFlowsJSON(G.table(nf, NAMES), REPORTER, RECEIVED, tls_names=tls, k8s=k8s, net=net, metrics=traced)
        direct.observe(tab, mrecs, k8s, net, REPORTER, features=(present, parts))
    assert traced.values == direct.values and traced.histograms == direct.histograms and len(traced.histograms) >= 2
    assert sum(v for (n, _), v in traced.values.items() if n == "namespace_flows_total") == len(mrecs) == len(lines[1]) - 1
    assert any(n == "namespace_drop_packets_total" for n, _ in traced.values) and any(n == "node_ipsec_flows_total" for n, _ in traced.values)


# ---- 2. the fold against a numpy group-by
def flow_columns(nf, spec, recs, present, parts):
    """Per flow what the spec's extra dimensions, value slots and bucket are, by the rules of include/nfagg.h, in numpy:
    (cause, state, rcode, ipsec, bucket, [value as Python ints], [has])."""
    L = nf._lib
    n = len(recs)
    parts = parts or {}
    have = lambda kind, bit: (np.asarray(present) & bit != 0) if present is not None and parts.get(kind) is not None else np.zeros(n, dtype=bool)  # noqa: E731
    zero = np.zeros(n, dtype=np.int64)
    ha, hd, hp = have("additional", 1), have("dns", 2), have("drops", 4)
    a = parts["additional"] if ha.any() else np.zeros(n, dtype=nf.ADDITIONAL)
    d = parts["dns"] if hd.any() else np.zeros(n, dtype=nf.DNS)
    p = parts["drops"] if hp.any() else np.zeros(n, dtype=nf.PKT_DROP)
    dns_ok, drop_ok = hd & (d["id"] != 0), hp & (p["latest_drop_cause"] != 0)
    lat = d["latency"].astype(np.uint64).view(np.int64)
    lat_ms = np.sign(lat) * (np.abs(lat.astype(object)) // 10**6)                                  # truncating toward zero, in Python integers
    b, pk = recs["metrics"]["bytes"].astype(np.uint64), recs["metrics"]["packets"].astype(np.uint64)
    sources = {L.MET_VALUE_RTT_NS: (a["flow_rtt"].astype(np.uint64).view(np.int64).astype(object), ha & (a["flow_rtt"] != 0)),
               L.MET_VALUE_DNS_LATENCY_MS: (lat_ms, dns_ok), L.MET_VALUE_DROP_BYTES: (p["bytes"].astype(object), drop_ok),
               L.MET_VALUE_DROP_PACKETS: (p["packets"].astype(object), drop_ok), L.MET_VALUE_BYTES: (b.astype(object), b != 0),
               L.MET_VALUE_PACKETS: (pk.astype(object), pk != 0)}
    xd = spec.get("xdims", 0)
    cause = np.where(drop_ok, p["latest_drop_cause"].astype(np.int64), 0) if xd & L.XDIM_DROP_CAUSE else zero
    state = np.where(drop_ok, p["latest_state"].astype(np.int64), 0xFFFF) if xd & L.XDIM_DROP_STATE else zero + 0xFFFF
    rcode = np.where(dns_ok, (d["flags"] & 0xF).astype(np.int64), 0xFF) if xd & L.XDIM_DNS_RCODE else zero + 0xFF
    ipsec = np.where(ha & (a["ipsec_encrypted_ret"] != 0), 2, np.where(ha & (a["ipsec_encrypted"] != 0), 1, 0)) if xd & L.XDIM_IPSEC_STATUS else zero
    values = [sources[s] for s in spec.get("value", ())]
    bucket = zero + L.MET_NO_BUCKET
    if spec.get("hist"):
        v, has = values[spec["hist"] - 1]
        bounds = list(spec["bounds"])
        bucket = np.array([next((k for k, bd in enumerate(bounds) if x <= bd), len(bounds)) if h else L.MET_NO_BUCKET for x, h in zip(v, has)], dtype=np.int64)
    return cause, state, rcode, ipsec, bucket, values


def numpy_groups(nf, spec, entries, layer, recs, k8s_rows, net_rows, present, parts):
    """test_flp_metrics_gpu.numpy_groups with the four extra key columns, the bucket and the value sums."""
    plain = MG.numpy_groups(nf, spec.get("dims", 0), entries, layer, recs, k8s_rows, net_rows)    # for the eight key columns, flow by flow, below
    L = nf._lib
    n = len(recs)
    key = np.zeros((n, 13), dtype=np.int64)
    dims = spec.get("dims", 0)
    for side in (0, 1):
        cls = MG.row_classes(entries, dims, side)
        if cls is not None and len(cls):
            r = k8s_rows[:, side].astype(np.int64)
            key[:, side] = np.where(r < len(entries), cls[np.minimum(r, len(entries) - 1)], 0)
    nr = net_rows if net_rows is not None else np.zeros(n, dtype=nf.NET_ROW)
    key[:, 2] = nr["src_label"] if dims & L.DIM_SRC_SUBNET_LABEL else L.NET_NO_LABEL
    key[:, 3] = nr["dst_label"] if dims & L.DIM_DST_SUBNET_LABEL else L.NET_NO_LABEL
    key[:, 4] = nr["direction"] if dims & L.DIM_FLOW_DIRECTION else L.NET_NO_DIRECTION
    if dims & L.DIM_FLOW_LAYER and layer is not None:
        app = np.array([K._b(info.get("namespace")) != b"" and K.object_is_app(K._b(info.get("namespace")), K._b(info.get("name")), layer) for _, info in entries] + [False])
        idx = np.minimum(k8s_rows.astype(np.int64), len(entries))
        key[:, 5] = np.where(app[idx[:, 0]] | app[idx[:, 1]], 2, 1)
    is_ip = np.isin(recs["metrics"]["eth_protocol"], (0x0800, 0x86DD))
    if dims & L.DIM_PROTO:
        key[:, 6], key[:, 7] = np.where(is_ip, recs["id"]["transport_protocol"], 0), is_ip
    cause, state, rcode, ipsec, bucket, values = flow_columns(nf, spec, recs, present, parts)
    key[:, 8], key[:, 9], key[:, 10], key[:, 11], key[:, 12] = cause, state, rcode, ipsec, bucket
    uniq, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    assert len(np.unique(key[:, :8], axis=0)) == len(plain)
    out = np.zeros(len(uniq), dtype=nf.METRIC_GROUP_CONTENT)
    for k, f in enumerate(KEY):
        out[f] = uniq[:, k]
    b, p = recs["metrics"]["bytes"].astype(np.uint64), recs["metrics"]["packets"].astype(np.uint64)
    for f, v in (("flows", np.ones(n, dtype=np.uint64)), ("bytes", b), ("packets", p), ("flows_with_bytes", (b != 0).astype(np.uint64)),
                 ("flows_with_packets", (p != 0).astype(np.uint64))):
        np.add.at(out[f], inv, v)
    for slot, (v, has) in enumerate(values):
        sums, counts = [0] * len(uniq), [0] * len(uniq)
        for i in np.flatnonzero(has):
            sums[inv[i]] += int(v[i])
            counts[inv[i]] += 1
        out["value_sum"][:, slot] = [s % 2**64 for s in sums]
        out["flows_with_value"][:, slot] = counts
    return out


def by_key(groups):
    return np.sort(groups, order=KEY)


def fold_both(nf, tab, met, recs, k8s_rows, net_rows, caps, present=None, parts=None):
    """The host call, then the device call into buffers of exactly the caps with 0xAB canaries over them and 128 bytes behind. Both
    must agree; returns (rc, groups sorted by key, n_groups)."""
    import torch
    n, G_ = len(recs), len(met.groupings)
    caps = [caps] * G_ if np.isscalar(caps) else list(caps)
    feats = (present, parts) if present is not None else None
    rc, groups, counts = tab.metrics_fold_content(met, recs, k8s_rows, net_rows, caps, feats)
    d_recs, d_k8s = (E.dev(recs), E.dev(k8s_rows)) if n else (None, None)
    d_net = E.dev(net_rows) if net_rows is not None and n else None
    d_feats, keep = None, []
    if feats is not None and n:
        keep = {k: E.dev(v) for k, v in parts.items() if k in ("additional", "dns", "drops", "xlat", "quic") and v is not None}
        d_present = E.dev(np.ascontiguousarray(present, dtype=np.uint8))
        d_feats = (d_present.data_ptr(), {k: v.data_ptr() for k, v in keep.items()})
    d_outs = [torch.full((c * 128 + 128,), 0xAB, dtype=torch.uint8, device="cuda") for c in caps]
    rc_d, counts_d = tab.metrics_fold_content_device(met, d_recs.data_ptr() if n else 0, n, d_k8s.data_ptr() if n else 0,
                                                     d_net.data_ptr() if d_net is not None else 0, caps, [o.data_ptr() for o in d_outs], d_feats)
    torch.cuda.synchronize()
    assert rc_d == rc
    for a, b, c in zip(counts, counts_d, caps):
        assert (a == b) if a <= c else (b > c)
    outs = []
    for g in range(G_):
        raw = d_outs[g].cpu().numpy()
        used = counts[g] * 128 if rc == nf.OK else 0
        assert (raw[used:] == 0xAB).all(), "grouping %d: bytes behind its groups were written" % g
        got = by_key(raw[:used].copy().view(nf.METRIC_GROUP_CONTENT))
        assert got.tobytes() == by_key(groups[g]).tobytes()
        assert (got["pad_"] == 0).all() and (got["pad2_"] == 0).all() and len(np.unique(got[KEY])) == len(got)
        outs.append(got)
    return rc, outs, counts


def check_fold(nf, tab, entries, layer, rules, specs, recs, present, parts, caps=4096):
    with tab.k8s_table(entries, layer) as k8s, NC.net_table(nf, rules, tab) as net, tab.metrics_table_specs(k8s, specs) as met:
        k8s_rows = tab.k8s_resolve(k8s, recs)
        net_rows = tab.net_resolve(net, recs, k8s, k8s_rows, REPORTER)
        rc, got, counts = fold_both(nf, tab, met, recs, k8s_rows, net_rows, caps, present, parts)
        assert rc == nf.OK
        for g, sp in enumerate(specs):
            if not len(recs):
                assert counts[g] == 0
                continue
            want = numpy_groups(nf, sp, entries, layer, recs, k8s_rows, net_rows, present, parts)
            assert counts[g] == len(want), "grouping %d: %d groups, not %d" % (g, counts[g], len(want))
            assert got[g].tobytes() == by_key(want).tobytes(), "grouping %d" % g
    return got


def eight_specs(nf):
    L = nf._lib
    d = lambda *keys: MG.dims_of(nf, *keys)  # noqa: E731
    rtt = (5_000_000, 10_000_000, 25_000_000, 50_000_000, 100_000_000, 250_000_000, 500_000_000, 1_000_000_000, 2_500_000_000, 5_000_000_000)
    return [dict(dims=d(*NS), value=(L.MET_VALUE_RTT_NS,), hist=1, bounds=rtt),
            dict(dims=d(*NS), xdims=L.XDIM_DNS_RCODE, value=(L.MET_VALUE_BYTES, L.MET_VALUE_DNS_LATENCY_MS), hist=2, bounds=(0, 0, 5, 50, 500, 5000)),
            dict(dims=d(*NS), xdims=L.XDIM_DROP_CAUSE | L.XDIM_DROP_STATE, value=(L.MET_VALUE_DROP_BYTES, L.MET_VALUE_DROP_PACKETS)),
            dict(dims=0), dict(dims=d("Proto", "FlowDirection", "K8S_FlowLayer")), dict(xdims=L.XDIM_ALL),
            dict(dims=L.DIM_ALL, xdims=L.XDIM_IPSEC_STATUS, value=(L.MET_VALUE_PACKETS,)), dict(dims=d("SrcSubnetLabel"), value=(L.MET_VALUE_RTT_NS, L.MET_VALUE_RTT_NS))]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_record_counts(nf, tab, world, n):
    recs, present, parts, entries, _ = world
    cut = {k: v[:n] for k, v in parts.items()}
    got = check_fold(nf, tab, entries, LAYER, ALL, eight_specs(nf)[:3], recs[:n], present[:n], cut)
    assert all((len(g) == 0) == (n == 0) for g in got)


def test_a_grid_stride_remainder(nf, tab, world):
    """A workgroup of 512 lanes per 4 096 flows: nine workgroups walk 33 545 flows in eight strides, the last one partial."""
    recs, present, parts, entries, _ = world
    n = 8 * 4096 + 777
    idx = np.arange(n) % len(recs)
    got = check_fold(nf, tab, entries, LAYER, ALL, eight_specs(nf)[:3], recs[idx], present[idx], {k: v[idx] for k, v in parts.items()})
    assert all(int(g["flows"].sum()) == n for g in got)


# ---- 3. a plain table, and no features
def test_a_plain_table_and_no_features_give_the_plain_fold(nf, tab, world):
    recs, present, parts, entries, _ = world
    groupings = MG.eight_groupings(nf)
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, ALL, tab) as net, tab.metrics_table(k8s, groupings) as plain, \
            tab.metrics_table_specs(k8s, [dict(dims=d) for d in groupings]) as specs:
        k8s_rows = tab.k8s_resolve(k8s, recs)
        net_rows = tab.net_resolve(net, recs, k8s, k8s_rows, REPORTER)
        rc, want, counts = tab.metrics_fold(plain, recs, k8s_rows, net_rows, 4096)
        assert rc == nf.OK
        for met, feats in ((plain, (present, parts)), (plain, None), (specs, None), (specs, (present, parts))):
            rc, got, counts_c = fold_both(nf, tab, met, recs, k8s_rows, net_rows, 4096, *(feats or (None, None)))
            assert rc == nf.OK and counts_c == counts
            for g in range(len(groupings)):
                w, c = MG.by_key(want[g]), got[g]
                assert c.view(np.uint8).reshape(-1, 128)[:, :16].tobytes() == w.view(np.uint8).reshape(-1, 64)[:, :16].tobytes()      # the key, byte for byte
                assert c.view(np.uint8).reshape(-1, 128)[:, 32:72].tobytes() == w.view(np.uint8).reshape(-1, 64)[:, 16:56].tobytes()  # the five sums
                assert (c["bucket"] == 0xFF).all() and (c["dns_rcode"] == 0xFF).all() and (c["drop_state"] == 0xFFFF).all()
                assert not c["drop_cause"].any() and not c["ipsec_status"].any() and not c["value_sum"].any() and not c["flows_with_value"].any()
        with pytest.raises(nf.NfaggError) as e:                                                 # the plain fold has no room for a spec table's groups
            tab.metrics_fold(specs, recs, k8s_rows, net_rows, 4096)
        assert e.value.code == nf._lib.EINVAL and "created from specs" in str(e.value)


# ---- 4. bucket edges
def plain_flows(nf, n, ip=("10.0.0.7", "10.0.2.200")):
    recs = np.resize(NG.ip_records(nf, [ip]), n)
    return recs, np.zeros(n, dtype=np.uint8), dict(additional=np.zeros(n, dtype=nf.ADDITIONAL), dns=np.zeros(n, dtype=nf.DNS), drops=np.zeros(n, dtype=nf.PKT_DROP))


@pytest.mark.parametrize("bounds", [(7,), tuple(range(-16, 16)), (I64_MIN,) + (-3,) * 4 + (0, 0, 0, 5, 5) + tuple(range(100, 2100, 100)) + (I64_MAX - 1, I64_MAX - 1),
                                    (I64_MIN,), (I64_MAX,)], ids=["one", "thirty-two", "equal neighbours", "min", "max"])
def test_bucket_edges(nf, tab, bounds):
    """An RTT of every bound, of every bound + 1, and of INT64_MIN, -1, 0 (no value: RTT 0 is no key), 1, INT64_MAX; a flow
    without the part. With equal neighbours the first of them takes the flows and the others stay empty."""
    L = nf._lib
    values = sorted({v for b in bounds for v in (b, min(b + 1, I64_MAX))} | {I64_MIN, -1, 0, 1, I64_MAX})
    recs, present, parts = plain_flows(nf, len(values) + 1)
    present[:-1] = 1
    parts["additional"]["flow_rtt"][:-1] = np.array([v % 2**64 for v in values], dtype=np.uint64)
    spec = dict(value=(L.MET_VALUE_RTT_NS,), hist=1, bounds=bounds)
    got = check_fold(nf, tab, [], None, R.RULES_OFF, [spec], recs, present, parts)[0]
    want = {}
    for v in values:
        if v != 0:
            k = next((k for k, b in enumerate(bounds) if v <= b), len(bounds))
            want[k] = want.get(k, 0) + 1
    want[L.MET_NO_BUCKET] = 2                                                                 # the RTT of 0 and the flow without the part
    assert dict(zip(got["bucket"].tolist(), got["flows"].tolist())) == want


def test_bytes_above_int64_go_to_inf(nf, tab):
    L = nf._lib
    recs, present, parts = plain_flows(nf, 6)
    recs["metrics"]["bytes"] = np.array([0, 1, 2**63 - 1, 2**63, 2**64 - 1, 10], dtype=np.uint64)
    spec = dict(value=(L.MET_VALUE_BYTES,), hist=1, bounds=(1, 10, I64_MAX))
    got = check_fold(nf, tab, [], None, R.RULES_OFF, [spec], recs, None, None)[0]
    assert dict(zip(got["bucket"].tolist(), got["flows"].tolist())) == {0: 1, 1: 1, 2: 1, 3: 2, L.MET_NO_BUCKET: 1}
    inf = got[got["bucket"] == 3][0]
    assert int(inf["value_sum"][0]) == (2**63 + 2**64 - 1) % 2**64 and int(inf["flows_with_value"][0]) == 2


# ---- 5. presence and arithmetic
def test_presence_and_arithmetic(nf, tab):
    L = nf._lib
    spec = dict(xdims=L.XDIM_ALL, value=(L.MET_VALUE_DNS_LATENCY_MS, L.MET_VALUE_DROP_PACKETS), hist=1, bounds=(-1, 0, 1000))
    lat = [5 * 10**6, 0, -1, -999_999, -1_000_000, 2**63, 2**64 - 1, 1_999_999, 10**15]
    recs, present, parts = plain_flows(nf, len(lat) + 8)
    d, p, a = parts["dns"], parts["drops"], parts["additional"]
    n = len(lat)
    present[:n] = 2
    d["latency"][:n], d["id"][:n], d["flags"][:n] = np.array([v % 2**64 for v in lat], dtype=np.uint64), 7, 0x8183        # rcode 3
    d["id"][0] = 0                                                             # a dns part with id 0: no value, rcode none
    d["latency"][n], d["id"][n] = 10**9, 7                                     # the part without its present bit
    present[n + 1], p["latest_drop_cause"][n + 1], p["packets"][n + 1], p["latest_state"][n + 1] = 4, 0, 9, 3             # drops with cause 0: none
    present[n + 2], p["latest_drop_cause"][n + 2], p["packets"][n + 2], p["latest_state"][n + 2] = 4, 2, 0, 0             # a cause, 0 packets, state 0: all real
    present[n + 3], p["latest_drop_cause"][n + 3], p["packets"][n + 3], p["latest_state"][n + 3] = 4, 2**32 - 1, 65535, 255
    present[n + 4], a["ipsec_encrypted_ret"][n + 4], a["ipsec_encrypted"][n + 4] = 1, -5, 1                               # error wins
    present[n + 5], a["ipsec_encrypted"][n + 5] = 1, 1
    present[n + 6] = 1                                                         # the part, neither flag: none
    present[n + 7] = 7
    got = check_fold(nf, tab, [], None, R.RULES_OFF, [spec], recs, present, parts)[0]
    row = lambda **kw: got[np.logical_and.reduce([got[k] == v for k, v in kw.items()])]  # noqa: E731
    dns = row(dns_rcode=3)
    ms = {int(b): (int(g["flows"]), int(g["value_sum"][0]) - (2**64 if int(g["value_sum"][0]) >> 63 else 0)) for b, g in zip(dns["bucket"], dns)}
    # 0, -1 and -999 999 ns are 0 ms, -1 000 000 ns is -1 ms; 2^63 is INT64_MIN ns; 2^64 - 1 is -1 ns: 0 ms
    assert ms == {0: (2, -1 - 2**63 // 10**6), 1: (4, 0), 2: (1, 1), 3: (1, 10**9)} and int(dns["flows_with_value"][:, 0].sum()) == 8
    assert len(row(drop_cause=0, drop_state=0xFFFF, dns_rcode=0xFF, ipsec_status=0, bucket=0xFF)) == 1
    assert int(row(drop_cause=0, drop_state=0xFFFF, dns_rcode=0xFF, ipsec_status=0, bucket=0xFF)["flows"][0]) == 5        # id 0, no bit, cause 0, no flag, nothing
    real = row(drop_cause=2, drop_state=0)
    assert len(real) == 1 and int(real["flows_with_value"][0][1]) == 1 and int(real["value_sum"][0][1]) == 0
    assert int(row(drop_cause=2**32 - 1, drop_state=255)["value_sum"][0][1]) == 65535
    assert int(row(ipsec_status=2)["flows"].sum()) == 1 and int(row(ipsec_status=1)["flows"].sum()) == 1
    # a NULL array with its present bit set is absent: the same flows without the dns array lose every DNS key
    none = check_fold(nf, tab, [], None, R.RULES_OFF, [spec], recs, present, dict(parts, dns=None))[0]
    assert (none["dns_rcode"] == 0xFF).all() and (none["bucket"] == 0xFF).all() and not none["flows_with_value"][:, 0].any()
    assert int(none["flows_with_value"][:, 1].sum()) == 2
    bare = check_fold(nf, tab, [], None, R.RULES_OFF, [spec], recs, None, None)[0]              # features == NULL: no flow has a part
    assert len(bare) == 1 and int(bare["flows"][0]) == len(recs)


# ---- 6. one hot (group, bucket)
def test_one_hot_group_and_bucket(nf, tab):
    """100 000 flows of one group and one bucket, 2^45 ns each: every lane adds to one slot, and the value sum passes 2^53."""
    L = nf._lib
    n = 100_000
    recs, present, parts = plain_flows(nf, n)
    present[:] = 1
    parts["additional"]["flow_rtt"] = 2**45
    entries = [("10.0.0.7", dict(namespace="shop", name="a", kind="Pod")), ("10.0.2.200", dict(namespace="shop", name="b", kind="Pod"))]
    spec = dict(dims=L.DIM_ALL, xdims=L.XDIM_ALL, value=(L.MET_VALUE_RTT_NS, L.MET_VALUE_PACKETS), hist=1, bounds=(2**44, 2**45, 2**46))
    got = check_fold(nf, tab, entries, LAYER, ALL, [spec], recs, present, parts)[0]
    assert len(got) == 1 and int(got["bucket"][0]) == 1 and int(got["value_sum"][0][0]) == n * 2**45 > 2**53
    assert got["flows_with_value"][0].tolist() == [n, n] and int(got["value_sum"][0][1]) == 3 * n and int(got["flows"][0]) == n


# ---- 7. more groups than any LDS table holds; truncation; caps
def test_large_fold_truncation_and_caps(nf, tab):
    """40 000 name pairs, each in four buckets: 160 000 groups go through the global table."""
    L = nf._lib
    base, entries = large_world(nf)
    recs = np.tile(base, 4)
    n = len(recs)
    present = np.ones(n, dtype=np.uint8)
    parts = dict(additional=np.zeros(n, dtype=nf.ADDITIONAL))
    parts["additional"]["flow_rtt"] = 1 + np.arange(n) // len(base)
    specs = [dict(dims=MG.dims_of(nf, "SrcK8S_Name", "DstK8S_Name"), value=(L.MET_VALUE_RTT_NS,), hist=1, bounds=(1, 2, 3)),
             dict(dims=MG.dims_of(nf, "SrcK8S_Namespace"), value=(L.MET_VALUE_RTT_NS,), hist=1, bounds=(1, 2, 3))]
    got = check_fold(nf, tab, entries, None, R.RULES_OFF, specs, recs, present, parts, caps=[1 << 18, 256])
    assert 4 * 39_000 < len(got[0]) <= 4 * 40_000 and len(got[1]) == 200 and set(got[0]["bucket"].tolist()) == {0, 1, 2, 3}
    with tab.k8s_table(entries) as k8s, tab.metrics_table_specs(k8s, specs) as met:
        k8s_rows = tab.k8s_resolve(k8s, recs)
        rc, out, counts = fold_both(nf, tab, met, recs, k8s_rows, None, [256, 256], present, parts)       # fold_both's canaries: nothing written
        assert rc == nf.TRUNCATED and counts[0] > 256 and counts[1] == 200 and len(out[0]) == 0 == len(out[1])
        exact = len(got[0])
        rc, out, counts = fold_both(nf, tab, met, recs, k8s_rows, None, [exact, 200], present, parts)     # caps of exactly the group counts
        assert rc == nf.OK and counts == [exact, 200]
        rc, out, counts = fold_both(nf, tab, met, recs, k8s_rows, None, [exact - 1, 200], present, parts)
        assert rc == nf.TRUNCATED and counts[0] > exact - 1 and counts[1] == 200
        rc, out, counts = fold_both(nf, tab, met, recs, k8s_rows, None, [exact, 199], present, parts)
        assert rc == nf.TRUNCATED and counts[0] == exact and counts[1] > 199
        with pytest.raises(nf.NfaggError) as e:
            tab.metrics_fold_content(met, recs, k8s_rows, None, [8, (1 << 20) + 1], (present, parts))
        assert e.value.code == L.ERANGE and "grouping 1: a cap of 1048577" in str(e.value)


def large_world(nf):
    """test_flp_metrics_gpu's `large` fixture, built here: 40 000 flows between 3 000 named rows."""
    rng = np.random.default_rng(97)
    n, rows = 40_000, 3_000
    addr = np.zeros((rows, 16), dtype=np.uint8)
    addr[:, 10:12], addr[:, 12], addr[:, 13], addr[:, 14], addr[:, 15] = 0xFF, 10, 77, np.arange(rows) >> 8, np.arange(rows) & 255
    entries = [(addr[k].tobytes(), dict(namespace="ns-%d" % (k % 50), name="obj-%d" % k, kind="Pod")) for k in range(rows)]
    recs = np.zeros(n, dtype=nf.FLOW_RECORD)
    recs["id"]["src_ip"], recs["id"]["dst_ip"] = addr[rng.integers(0, rows, n)], addr[rng.integers(0, rows, n)]
    recs["metrics"]["eth_protocol"], recs["id"]["transport_protocol"] = 0x0800, 6
    recs["metrics"]["bytes"], recs["metrics"]["packets"] = rng.integers(0, 2**40, n), rng.integers(0, 100, n)
    return recs, entries


# ---- 8. eight specs in one call
def test_eight_specs_in_one_call_give_what_each_gives_alone(nf, tab, world):
    recs, present, parts, entries, _ = world
    specs = eight_specs(nf)
    together = check_fold(nf, tab, entries, LAYER, ALL, specs, recs, present, parts)
    for g, sp in enumerate(specs):
        alone = check_fold(nf, tab, entries, LAYER, ALL, [sp], recs, present, parts)[0]
        assert alone.tobytes() == together[g].tobytes(), g
    assert len(together[3]) == 1 and int(together[3]["flows"][0]) == len(recs) and len(together[5]) > 30 and len(together[0]) > len(np.unique(together[0][KEY[:8]]))
    assert (together[7]["value_sum"][:, 0] == together[7]["value_sum"][:, 1]).all()           # one source in both slots


# ---- 9. crafted keys: one (A, B), one home slot, third words that differ
def test_keys_that_differ_in_their_third_word_alone_on_one_slot(nf, tab):
    """Twenty drop causes whose keys (one class pair, one second word) share the low ten bits of nfagg_metrics_group_hash_content,
    found by search as tests/keycraft.py's helpers find theirs: one home slot in the LDS table of either size and in a global table
    of 1 024 slots, so the probe walks past slots that hold the same (A, B) with another C, and past kMetLdsProbe of them into the
    global table. Each cause comes in five more keys that differ from the crafted one in the state or the bucket alone: they
    land elsewhere and must not merge."""
    L = nf._lib
    template = np.zeros(1, dtype=nf.METRIC_GROUP_CONTENT)
    template["src_label"], template["dst_label"], template["direction"] = L.NET_NO_LABEL, L.NET_NO_LABEL, L.NET_NO_DIRECTION
    template["dns_rcode"], template["drop_state"] = 0xFF, 1
    template["bucket"] = 2                                                 # the crafted keys: state 1, two packets (the third bucket)
    cand = np.repeat(template, 60_000)
    cand["drop_cause"] = np.arange(1, 60_001)
    h = nf.metrics_group_hash_content(0, cand)
    home, count = np.unique(h & np.uint64(1023), return_counts=True)
    causes = cand["drop_cause"][(h & np.uint64(1023)) == home[np.argmax(count)]][:20]
    assert len(causes) == 20
    variants = np.array([(1, 2), (2, 2), (1, 0), (1, 1), (1, 3), (1, 4)])    # (state, packets): the crafted one, then keys that land elsewhere
    reps = 37
    recs, present, parts = plain_flows(nf, len(causes) * len(variants) * reps)
    present[:] = 4
    p = parts["drops"]
    p["latest_drop_cause"] = np.tile(np.repeat(causes, len(variants)), reps)
    p["latest_state"] = np.tile(variants[:, 0], len(causes) * reps)
    p["bytes"], p["packets"] = 1000, np.tile(variants[:, 1], len(causes) * reps)
    spec = dict(xdims=L.XDIM_DROP_CAUSE | L.XDIM_DROP_STATE, value=(L.MET_VALUE_DROP_BYTES, L.MET_VALUE_DROP_PACKETS), hist=2, bounds=(0, 1, 2, 3))
    got = check_fold(nf, tab, [], None, R.RULES_OFF, [spec], recs, present, parts, caps=512)[0]
    assert len(got) == len(causes) * len(variants) and int(got["flows"].sum()) == len(recs) and (got["flows"] == reps).all()
    assert set(got["drop_cause"].tolist()) == set(causes.tolist()) and set(got["bucket"].tolist()) == {0, 1, 2, 3, 4}
    crafted = got[(got["drop_state"] == 1) & (got["bucket"] == 2)]
    assert len(np.unique(nf.metrics_group_hash_content(0, crafted) & np.uint64(1023))) == 1 and len(crafted) == 20
    with tab.k8s_table([]) as k8s, tab.metrics_table_specs(k8s, [spec]) as met:                  # the crafted keys against a cap of exactly their number
        rows = tab.k8s_resolve(k8s, recs)
        assert fold_both(nf, tab, met, recs, rows, None, [len(got)], present, parts)[0] == nf.OK
        assert fold_both(nf, tab, met, recs, rows, None, [len(got) - 1], present, parts)[0] == nf.TRUNCATED
