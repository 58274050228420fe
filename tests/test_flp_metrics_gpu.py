"""Flow metrics on the GPU (nfagg_metrics_fold, csrc/nfagg_metrics.hip) through the C ABI, host and device entry points:
PromCounters.observe against the per-flow restatement of tests/flp_metrics_ref.py on the seeded streams of the direct-FLP tests,
and the fold itself against a numpy group-by of the resolved rows: sizes, groups that share a key half, eight groupings in one
call, one hot group, tens of thousands of groups, overflow, caps, classes. Records, informer answers, layer rule and subnet
categories are those of tests/test_flp_json_net_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_k8s_ref as K  # noqa: E402
import flp_json_net_ref as R  # noqa: E402
import flp_metrics_ref as M  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_flp_json_k8s_gpu as KG  # noqa: E402
import test_flp_json_net_cpu as NC  # noqa: E402
import test_flp_json_net_gpu as NG  # noqa: E402
import test_netev_gpu as E  # noqa: E402
from flp_json_ref import record_to_map  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, NOW, MONO, RECEIVED = G.NAMES, G.NOW, G.MONO, G.RECEIVED
LAYER, INFOS, CATEGORIES, REPORTER, ALL = KG.LAYER, KG.INFOS, NG.CATEGORIES, NG.REPORTER, NG.ALL
FIELDS = K.FIELDS

# all six filter types, two filters on one key, remap, the three value keys, valueScale 0 / 1 / 1000; `by_layer` and `to_pods`
# filter on keys they do not label by
ITEMS = [
    dict(name="namespace_flows_total", type="counter", labels=["SrcK8S_Namespace", "DstK8S_Namespace", "K8S_FlowLayer", "SrcSubnetLabel", "DstSubnetLabel"],
         remap={"K8S_FlowLayer": "layer", "SrcSubnetLabel": ""}),
    dict(name="workload_bytes_total", type="counter", valueKey="Bytes", valueScale=1,
         labels=["SrcK8S_OwnerName", "SrcK8S_OwnerType", "SrcK8S_Namespace", "DstK8S_OwnerName", "DstK8S_OwnerType", "DstK8S_Namespace", "FlowDirection"]),
    dict(name="by_layer", type="counter", valueKey="Bytes", labels=["DstK8S_Namespace"], filters=[dict(key="K8S_FlowLayer", value="app", type="equal")]),
    dict(name="node_kpackets_total", type="counter", valueKey="Packets", valueScale=1000, labels=["SrcK8S_HostName", "DstK8S_HostName", "Proto"],
         filters=[dict(key="Proto", value="^(6|17)$", type="match_regex"), dict(key="SrcK8S_HostIP", type="presence")]),
    dict(name="to_pods", type="counter", labels=["SrcK8S_Type"],
         filters=[dict(key="DstK8S_Type", value="Pod", type="equal"), dict(key="DstK8S_Type", value="Service", type="equal"),
                  dict(key="SrcK8S_Namespace", value="openshift", type="not_match_regex"), dict(key="DstK8S_Zone", type="absence")]),
    dict(name="not_inner_packets", type="counter", valueKey="Packets", labels=["FlowDirection", "SrcK8S_Zone"], remap={"FlowDirection": "direction"},
         filters=[dict(key="FlowDirection", value="2", type="not_equal")]),
    dict(name="same_node", type="counter", labels=["SrcK8S_HostIP"], filters=[dict(key="SrcK8S_HostIP", value="$(DstK8S_HostIP)")]),
    dict(name="flows_total", type="counter"),
]
SCALE = {"netobserv_" + it["name"]: it.get("valueScale", 0) for it in ITEMS}


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


def stream(nf, O, n, seed):
    """test_flp_json_gpu.stream with its byte counts bounded: the device's sums are 64-bit integers (modulo 2^64, include/nfagg.h),
    and two of the stream's records of 2^64 - 1 bytes would wrap a group's sum, which the reference's floats do not. 2^58 keeps
    every sum of a few hundred flows below 2^64 and far above 2^53, where a float addition rounds."""
    recs = G.stream(nf, O, n, seed)
    recs["metrics"]["bytes"] = np.minimum(recs["metrics"]["bytes"], np.uint64(2**58))
    return recs


@pytest.fixture(scope="module")
def world(nf, O):
    """300 flows of the seeded stream (v4, v6, non-IP records, zero bytes and packets), the informer answers for half of its
    addresses, and the restatement's answer: per flow the enriched map, the series as running floats and as exact integers."""
    recs = stream(nf, O, 300, 61)
    entries = KG.entries_for(recs)
    table, cats, names = K.table_of(entries), R.parse_subnets(CATEGORIES), G.rows(NAMES)
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 144)
    maps, memo = [], {}
    for i in range(len(raw)):
        m = record_to_map(raw[i].tobytes(), NOW, MONO, names, REPORTER, RECEIVED, b"unknown", memo)
        maps.append(R.apply_rules(m, table, LAYER, ALL, cats))
    return recs, entries, maps


def restate(maps, items=ITEMS):
    """(running float sums, exact integer sums) per series, the second by the restatement's own filters and labels."""
    ref = M.Counters(items, prefix="netobserv_")
    exact = {}
    for m in maps:
        ref.encode(m)
        for pre in ref.pre:
            if M.apply_filters(m, pre) and M.extract_generic_value(m, pre) is not None:
                key = ("netobserv_" + pre["name"], M.extract_labels(m, pre))
                exact[key] = exact.get(key, 0) + int(M.extract_generic_value(m, pre))
    return ref.values, exact


def check_counters(got: dict, maps, items=ITEMS, calls=None):
    """calls: the slices of `maps` that went into one observe() each (default: one call). A call adds float(exact sum) / scale to a
    series, so the value is known exactly; the restatement's one addition per flow agrees within n roundings."""
    floats, _ = restate(maps, items)
    want = {}
    for part in calls or [slice(0, len(maps))]:
        for key, total in restate(maps[part], items)[1].items():
            scale = SCALE.get(key[0], 0)
            want[key] = want.get(key, 0.0) + (float(total) / scale if scale else float(total))      # one rounding of the call's exact sum
    assert set(got) == set(floats) == set(want)
    for key in want:
        assert got[key] == want[key], key
        assert abs(got[key] - floats[key]) <= len(maps) * 2.0**-52 * abs(floats[key]), key   # n rounded additions
    return floats


# ---- parity with the per-flow restatement
def test_prom_counters_against_the_restatement(nf, tab, world):
    recs, entries, maps = world
    p = nf.PromCounters(ITEMS, prefix="netobserv_")
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, ALL, tab) as net:
        p.observe(tab, recs, k8s, net, REPORTER)
        once = dict(p.values)
        floats = check_counters(once, maps)
        p.observe(tab, recs, k8s, net, REPORTER)                                           # a second eviction adds to the same series
        assert p.values == {k: v + v for k, v in once.items()}
    count = {it["name"]: sum(1 for name, _ in floats if name == "netobserv_" + it["name"]) for it in ITEMS}
    print("series per metric:", count)
    assert all(c >= 1 for c in count.values()) and count["namespace_flows_total"] >= 3 and count["workload_bytes_total"] >= 3    # every metric has series
    assert any(v > 2.0**53 for (name, _), v in floats.items() if name == "netobserv_workload_bytes_total")
    assert floats[("netobserv_flows_total", ())] == 300.0
    assert any(dict(labels)["SrcSubnetLabel"] != b"" for name, labels in floats if name == "netobserv_namespace_flows_total")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_record_counts(nf, tab, world, n):
    recs, entries, maps = world
    p = nf.PromCounters(ITEMS, prefix="netobserv_")
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, ALL, tab) as net:
        p.observe(tab, recs[:n], k8s, net, REPORTER)
    check_counters(p.values, maps[:n])
    assert (len(p.values) == 0) == (n == 0)


def test_exporter_and_map_tracer_feed_the_counters(nf, O, tab, world):
    import io
    recs, entries, maps = world
    p = nf.PromCounters(ITEMS, prefix="netobserv_")
    out = io.BytesIO()
    with tab.tls_names() as tls, tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, ALL, tab) as net:
        exp = nf.StartDirectFLPJSON(tab, out, names=G.table(nf, NAMES), agent_ip=REPORTER, time_received=lambda: RECEIVED, tls_names=tls, k8s=k8s, net=net,
                                    metrics=p)
        assert exp.ExportEvicted(recs[:120], NOW, MONO) == 120 and exp.ExportEvicted(recs[120:], NOW, MONO) == 180
        check_counters(p.values, maps, calls=[slice(0, 120), slice(120, 300)])
        assert out.getvalue().count(b"\n") == 300

        from test_map_merge import make_maps                                                # the tracer observes the flows it merged
        main_ids, main_vals, feats = make_maps(O, seed=11, n_pop=400, n_main=300, n_feat=250, n_cpu=4)
        main_vals["eth_protocol"] = 0x86DD
        mrecs = tab.map_merge(main_ids, main_vals, feats, 4)[0]
        mt = nf.MapTracer(nf.GPUMapFetcher(tab, lambda: (main_ids, main_vals, feats, 4)), 0, 0, clock=lambda: NOW, mono_clock=lambda: MONO)
        traced, direct = nf.PromCounters(ITEMS), nf.PromCounters(ITEMS)
        lines = mt.evictFlowsJSON(G.table(nf, NAMES), REPORTER, RECEIVED, tls_names=tls, k8s=k8s, net=net, metrics=traced)
        direct.observe(tab, mrecs, k8s, net, REPORTER)
        assert traced.values == direct.values and traced.values[("flows_total", ())] == len(mrecs) == len(lines[1]) - 1


# ---- the fold against a numpy group-by of the resolved rows
def row_classes(entries, dims, side):
    """Per row the dense id, from 1 in order of first appearance, of its selected (text, presence) tuple; None: nothing selected."""
    sel = (dims >> (9 * side)) & 0x1FF
    if not sel:
        return None
    seen, out = {}, []
    for _, info in entries:
        t = {f: K._b(info.get(f)) for f in FIELDS}
        present = dict(namespace=t["namespace"] != b"", host_ip=t["host_ip"] != b"", host_name=t["host_ip"] != b"" and t["host_name"] != b"",
                       zone=info.get("zone") is not None)
        key = tuple((t[f], True) if present.get(f, True) else (b"", False) for k, f in enumerate(FIELDS) if sel >> k & 1)
        out.append(seen.setdefault(key, len(seen) + 1))
    return np.array(out, dtype=np.uint32)


def numpy_groups(nf, dims, entries, layer, recs, k8s_rows, net_rows):
    """The groups of one grouping, sorted by key: classes by row_classes, the layer from the rows' app flags, sums by np.add.at."""
    L = nf._lib
    n = len(recs)
    key = np.zeros((n, 8), dtype=np.int64)
    for side in (0, 1):
        cls = row_classes(entries, dims, side)
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
    uniq, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    out = np.zeros(len(uniq), dtype=nf.METRIC_GROUP)
    for k, f in enumerate(("src_class", "dst_class", "src_label", "dst_label", "direction", "layer", "proto", "is_ip")):
        out[f] = uniq[:, k]
    b, p = recs["metrics"]["bytes"].astype(np.uint64), recs["metrics"]["packets"].astype(np.uint64)
    for f, v in (("flows", np.ones(n, dtype=np.uint64)), ("bytes", b), ("packets", p), ("flows_with_bytes", (b != 0).astype(np.uint64)),
                 ("flows_with_packets", (p != 0).astype(np.uint64))):
        np.add.at(out[f], inv, v)
    return out


def by_key(groups):
    return np.sort(groups, order=["src_class", "dst_class", "src_label", "dst_label", "direction", "layer", "proto", "is_ip"])


def fold_both(nf, tab, met, recs, k8s_rows, net_rows, caps):
    """The host call, then the device call into buffers of exactly the caps with 0xAB canaries over them and 64 bytes behind. Both
    must agree; returns (rc, groups sorted by key, n_groups)."""
    import torch
    n, G_ = len(recs), len(met.groupings)
    caps = [caps] * G_ if np.isscalar(caps) else list(caps)
    rc, groups, counts = tab.metrics_fold(met, recs, k8s_rows, net_rows, caps)
    d_recs, d_k8s = (E.dev(recs), E.dev(k8s_rows)) if n else (None, None)
    d_net = E.dev(net_rows) if net_rows is not None and n else None
    d_outs = [torch.full((c * 64 + 64,), 0xAB, dtype=torch.uint8, device="cuda") for c in caps]
    rc_d, counts_d = tab.metrics_fold_device(met, d_recs.data_ptr() if n else 0, n, d_k8s.data_ptr() if n else 0, d_net.data_ptr() if d_net is not None else 0,
                                             caps, [o.data_ptr() for o in d_outs])
    torch.cuda.synchronize()
    assert rc_d == rc
    for a, b, c in zip(counts, counts_d, caps):                            # exact where the grouping fits, above the cap in both calls where not
        assert (a == b) if a <= c else (b > c)
    outs = []
    for g in range(G_):
        raw = d_outs[g].cpu().numpy()
        used = counts[g] * 64 if rc == nf.OK else 0
        assert (raw[used:] == 0xAB).all(), "grouping %d: bytes behind its groups were written" % g
        got = by_key(raw[:used].copy().view(nf.METRIC_GROUP))
        assert got.tobytes() == by_key(groups[g]).tobytes()
        assert (got["pad_"] == 0).all() and len(np.unique(got[["src_class", "dst_class", "src_label", "dst_label", "direction", "layer", "proto", "is_ip"]])) == len(got)
        outs.append(got)
    return rc, outs, counts


def check_fold(nf, tab, entries, layer, rules, groupings, recs, caps=4096, agent=REPORTER):
    with tab.k8s_table(entries, layer) as k8s, NC.net_table(nf, rules, tab) as net, tab.metrics_table(k8s, groupings) as met:
        k8s_rows = tab.k8s_resolve(k8s, recs)
        net_rows = tab.net_resolve(net, recs, k8s, k8s_rows, agent)
        rc, got, counts = fold_both(nf, tab, met, recs, k8s_rows, net_rows, caps)
        assert rc == nf.OK
        want = [numpy_groups(nf, d, entries, layer, recs, k8s_rows, net_rows) for d in groupings]
        for g, d in enumerate(groupings):
            assert counts[g] == len(want[g]) and got[g].tobytes() == by_key(want[g]).tobytes(), "grouping %d (0x%x)" % (g, d)
            for side, f in ((0, "src_class"), (1, "dst_class")):                            # a class names a row of that class
                cls = row_classes(entries, d, side)
                for c in np.unique(got[g][f]):
                    row = met.class_row(g, side, int(c))
                    assert (row == nf._lib.K8S_NO_ROW) if c == 0 else (cls[row] == c and row == int(np.flatnonzero(cls == c)[0]))
    return got


def dims_of(nf, *keys):
    d = 0
    for k in keys:
        d |= nf.metrics.KEY_DIMS[k]
    return d


def eight_groupings(nf):
    return [dims_of(nf, "SrcK8S_Namespace", "DstK8S_Namespace", "K8S_FlowLayer", "SrcSubnetLabel", "DstSubnetLabel"),
            dims_of(nf, "SrcK8S_OwnerName", "SrcK8S_OwnerType", "SrcK8S_Namespace", "DstK8S_OwnerName", "DstK8S_OwnerType", "DstK8S_Namespace", "FlowDirection"),
            0, dims_of(nf, "Proto"), dims_of(nf, "SrcK8S_Zone", "DstK8S_HostName"), nf._lib.DIM_ALL, dims_of(nf, "DstK8S_Name", "Proto", "FlowDirection"),
            dims_of(nf, "K8S_FlowLayer")]


def test_eight_groupings_in_one_call_give_what_each_gives_alone(nf, O, tab):
    recs = stream(nf, O, 1500, 83)
    entries = KG.entries_for(recs)
    groupings = eight_groupings(nf)
    together = check_fold(nf, tab, entries, LAYER, ALL, groupings, recs)
    for g, d in enumerate(groupings):
        alone = check_fold(nf, tab, entries, LAYER, ALL, [d], recs)[0]
        assert alone.tobytes() == together[g].tobytes(), g
    assert len(together[2]) == 1 and together[2]["flows"][0] == 1500 and len(together[5]) > 100 and {0, 1} == set(together[3]["is_ip"].tolist())
    assert len(check_fold(nf, tab, entries, None, R.RULES_OFF, groupings, recs)[7]) == 1      # no layer, no rule: every dimension at its "none"


def test_a_grid_stride_remainder(nf, O, tab):
    """A workgroup of 512 lanes per 4 096 flows: 65 workgroups walk 262 921 flows in eight strides, the last one partial."""
    base = stream(nf, O, 4099, 89)
    recs = np.resize(base, 512 * 512 + 777)
    got = check_fold(nf, tab, KG.entries_for(base), LAYER, ALL, eight_groupings(nf)[:2], recs)
    assert int(got[0]["flows"].sum()) == len(recs) == int(got[1]["flows"].sum())


def test_groups_that_share_their_first_key_half(nf, tab):
    """Four addresses whose rows carry one name (one class) in four subnets, every pair, five protocols: groups of one class pair
    that differ in labels, direction or protocol, and two groupings with the same mask in one call, whose keys differ in the
    grouping's index alone."""
    ips = ["10.0.0.7", "10.0.2.200", "2001:db8::1", "9.9.9.9"]
    hosts = ["192.168.1.10", "192.168.1.10", "192.168.1.11", ""]
    entries = [(ip, dict(namespace="shop", name="same", kind="Pod", host_ip=h)) for ip, h in zip(ips, hosts)]
    pairs = [(s, d) for s in ips for d in ips] * 5
    recs = NG.ip_records(nf, pairs)
    recs["id"]["transport_protocol"] = np.repeat(np.array([6, 17, 1, 58, 132], dtype=np.uint8), 16)
    recs["metrics"]["bytes"] = np.arange(len(recs)) * 1000
    one = dims_of(nf, "SrcK8S_Name", "DstK8S_Name", "SrcSubnetLabel", "DstSubnetLabel", "Proto")
    got = check_fold(nf, tab, entries, LAYER, ALL, [one, one, dims_of(nf, "SrcK8S_Name", "DstK8S_Name", "FlowDirection")], recs)
    assert got[0].tobytes() == got[1].tobytes() and set(got[0]["src_class"].tolist()) == {1} == set(got[0]["dst_class"].tolist())
    assert len(got[0]) == 5 * 16 and (got[0]["flows"] == 1).all() and len(got[2]) == 4 and set(got[2]["direction"].tolist()) == {0, 1, 2, 0xFF}


def test_one_hot_group(nf, tab):
    """100 000 flows of one group, 2^45 bytes each: every lane adds to one slot, and the byte sum passes 2^53."""
    n = 100_000
    recs = np.resize(NG.ip_records(nf, [("10.0.0.7", "10.0.2.200")]), n)
    recs["metrics"]["bytes"], recs["metrics"]["packets"] = 2**45, 3
    recs["metrics"]["packets"][::4] = 0
    entries = [("10.0.0.7", dict(namespace="shop", name="a", kind="Pod")), ("10.0.2.200", dict(namespace="shop", name="b", kind="Pod"))]
    got = check_fold(nf, tab, entries, LAYER, ALL, [nf._lib.DIM_ALL], recs)[0]
    assert len(got) == 1 and int(got["bytes"][0]) == n * 2**45 > 2**53
    assert (int(got["flows"][0]), int(got["packets"][0]), int(got["flows_with_bytes"][0]), int(got["flows_with_packets"][0])) == (n, 3 * (n - n // 4), n, n - n // 4)


@pytest.fixture(scope="module")
def large(nf):
    """40 000 flows between 3 000 named rows: tens of thousands of (src name, dst name) groups."""
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


def test_large_fold_more_groups_than_any_lds_table_holds(nf, tab, large):
    recs, entries = large
    got = check_fold(nf, tab, entries, None, R.RULES_OFF, [dims_of(nf, "SrcK8S_Name", "DstK8S_Name"), dims_of(nf, "SrcK8S_Namespace")], recs, caps=[65536, 64])
    assert 39_000 < len(got[0]) <= 40_000 and len(got[1]) == 50


def test_overflow(nf, tab, large):
    """Ten groups against a cap of 4: NFAGG_TRUNCATED, nothing written (fold_both's canaries cover the whole outputs), a count above
    the cap; the grouping that fits reports its exact count in the failed call. Then a grouping whose table fills up."""
    ips = ["10.0.0.%d" % k for k in range(1, 11)]
    entries = [(ip, dict(namespace="shop", name="pod-%d" % k, kind="Pod")) for k, ip in enumerate(ips)]
    recs = NG.ip_records(nf, [(ip, "10.0.0.1") for ip in ips] * 3)
    groupings = [dims_of(nf, "SrcK8S_Name"), dims_of(nf, "DstK8S_Name", "SrcK8S_Namespace")]
    with tab.k8s_table(entries) as k8s, tab.metrics_table(k8s, groupings) as met:
        k8s_rows = tab.k8s_resolve(k8s, recs)
        rc, got, counts = fold_both(nf, tab, met, recs, k8s_rows, None, [4, 4])
        assert rc == nf.TRUNCATED and counts[0] > 4 and counts[1] == 1 and len(got[0]) == 0 == len(got[1])
        rc, got, counts = fold_both(nf, tab, met, recs, k8s_rows, None, [16, 4])
        assert rc == nf.OK and counts == [10, 1] and (got[0]["flows"] == 3).all() and got[1]["flows"][0] == 30
        rc, got, counts = fold_both(nf, tab, met, recs, k8s_rows, None, [10, 1])             # caps of exactly the group counts
        assert rc == nf.OK and counts == [10, 1]
        rc, got, counts = fold_both(nf, tab, met, recs, k8s_rows, None, [9, 1])
        assert rc == nf.TRUNCATED and counts[0] > 9 and counts[1] == 1
        rc, got, counts = fold_both(nf, tab, met, recs, k8s_rows, None, [0, 0])
        assert rc == nf.TRUNCATED and counts[0] > 0 and counts[1] > 0
    recs, entries = large                                                                  # 40 000 groups against the smallest table
    groupings = [dims_of(nf, "SrcK8S_Name", "DstK8S_Name"), dims_of(nf, "SrcK8S_Namespace")]
    with tab.k8s_table(entries) as k8s, tab.metrics_table(k8s, groupings) as met:
        k8s_rows = tab.k8s_resolve(k8s, recs)
        rc, got, counts = fold_both(nf, tab, met, recs, k8s_rows, None, [256, 64])
        assert rc == nf.TRUNCATED and counts[0] > 256 and counts[1] == 50


def test_caps_and_arguments(nf, O, tab):
    L = nf._lib
    recs = stream(nf, O, 64, 53)
    with tab.k8s_table(KG.entries_for(recs), LAYER) as k8s, tab.metrics_table(k8s, [L.DIM_PROTO, L.DIM_SRC_SUBNET_LABEL]) as met, \
            tab.metrics_table(k8s, [L.DIM_PROTO]) as plain, nf.K8sTable([]) as host_k8s, nf.MetricsTable(host_k8s, [0]) as host_met:
        k8s_rows = tab.k8s_resolve(k8s, recs)
        with pytest.raises(nf.NfaggError) as e:
            tab.metrics_fold(met, recs, k8s_rows, None, [8, (1 << 20) + 1])
        assert e.value.code == L.ERANGE and "grouping 1: a cap of 1048577" in str(e.value)
        with pytest.raises(nf.NfaggError) as e:
            tab.metrics_fold(met, recs, k8s_rows, None, 64)
        assert e.value.code == L.EINVAL and "grouping 1 selects a label or the direction" in str(e.value)
        rc, groups, counts = tab.metrics_fold(plain, recs, k8s_rows, None, 64)             # no such dimension: no net rows needed
        assert rc == nf.OK and counts[0] == len(groups[0]) > 3 and int(groups[0]["flows"].sum()) == 64
        rc, groups, counts = tab.metrics_fold(met, recs[:0], k8s_rows[:0], None, 0)        # n == 0: no groups, whatever the caps
        assert rc == nf.OK and counts == [0, 0]
        with pytest.raises(nf.NfaggError) as e:
            tab.metrics_fold(host_met, recs, k8s_rows, None, 64)
        assert e.value.code == L.EINVAL and "metrics table was not created for this handle" in str(e.value)
        with pytest.raises(nf.NfaggError) as e:
            tab.metrics_table(host_k8s, [0])
        assert e.value.code == L.EINVAL and "Kubernetes table was not created for this handle" in str(e.value)
    p = nf.PromCounters([dict(name="l", type="counter", labels=["SrcSubnetLabel"])])
    with tab.k8s_table([]) as k8s, pytest.raises(ValueError):
        p.observe(tab, recs, k8s)


def test_prom_counters_grow_a_cap_and_retry(nf, tab, large):
    recs, entries = large
    items = [dict(name="pairs", type="counter", valueKey="Bytes", labels=["SrcK8S_Name", "DstK8S_Name"])]
    p = nf.PromCounters(items)
    assert p.caps == [4096]
    with tab.k8s_table(entries) as k8s:
        p.observe(tab, recs[:12_000], k8s)
    assert 11_900 < len(p.values) <= 12_000 and p.caps[0] >= 2 * len(p.values) > 4096
    assert sum(int(v) for v in p.values.values()) == int(recs["metrics"]["bytes"][:12_000].astype(object).sum())     # each group's sum is below 2^53


def test_classes_on_a_device_table(nf, tab):
    L = nf._lib
    entries = [("10.1.0.1", dict(namespace="a", name="x", kind="Pod", zone="")), ("10.1.0.2", dict(namespace="a", name="y", kind="Pod", zone="")),
               ("10.1.0.3", dict(namespace="a", name="x", kind="Pod")), ("10.1.0.4", dict(namespace="a", name="x", kind="Pod", zone="z"))]
    with tab.k8s_table(entries) as k8s, tab.metrics_table(k8s, [L.DIM_SRC_K8S(0) | L.DIM_SRC_K8S(8), L.DIM_DST_K8S(1)]) as met:
        assert met.n_classes(0, 0) == 3 and met.n_classes(0, 1) == 0 and met.n_classes(1, 1) == 2
        assert [met.class_row(0, 0, c) for c in (0, 1, 2, 3)] == [L.K8S_NO_ROW, 0, 2, 3]      # rows 0 and 1 differ in the name only; "" is not "no zone"
        recs = NG.ip_records(nf, [("10.1.0.1", "10.1.0.2"), ("10.1.0.2", "10.1.0.1"), ("10.1.0.3", "10.1.0.3"), ("10.1.0.4", "10.9.9.9")])
        rc, groups, counts = tab.metrics_fold(met, recs, tab.k8s_resolve(k8s, recs), None, 8)
        got = by_key(groups[0])
        assert rc == nf.OK and got["src_class"].tolist() == [1, 2, 3] and got["flows"].tolist() == [2, 1, 1] and (got["dst_class"] == 0).all()
        assert by_key(groups[1])["dst_class"].tolist() == [0, 1, 2]
