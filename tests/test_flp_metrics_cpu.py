"""Flow metrics, CPU side: the per-flow restatement of tests/flp_metrics_ref.py against the hand-worked vectors of
tests/golden/metrics_vectors.json; PromCounters' validation errors and grouping derivation; its per-group evaluation, fed with
hand-built group arrays and a host-only metrics table, against the restatement; tools/c/metrics_host_check.c compiled and run
against the library (no handle); the ABI's new symbols and the group's layout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_metrics_ref as M  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "metrics_vectors.json")))["cases"]


def flow_map(d: dict) -> dict:
    """A vector's flow as the restatements hold it: bytes keys, bytes or int values."""
    return {k.encode(): v.encode() if isinstance(v, str) else v for k, v in d.items()}


def series(values: dict, name: str) -> dict:
    """{frozenset of (target, value bytes): float} of one metric."""
    return {frozenset(labels): v for (n, labels), v in values.items() if n == name}


def wanted(case) -> dict:
    return {frozenset((k, v.encode()) for k, v in labels.items()): float(value) for labels, value in case["want"]}


# ---- the restatement against the vectors
@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"][:40] for c in GOLDEN])
def test_restatement_against_the_vectors(case):
    c = M.Counters([case["item"]], prefix="p_")
    for f in case["flows"]:
        c.encode(flow_map(f))
    assert series(c.values, "p_" + case["item"]["name"]) == wanted(case)
    assert len(GOLDEN) >= 12


def test_convert_to_string():
    assert M.convert_to_string(0) == b"0" and M.convert_to_string(2**64 - 1) == b"18446744073709551615" and M.convert_to_string(b"x\xff") == b"x\xff"


# ---- PromCounters: validation, groupings
@pytest.mark.parametrize("item, message", [
    (dict(name="g", type="gauge"), "is not counter"),
    (dict(name="h", type="histogram", valueKey="Bytes"), "is not counter"),
    (dict(name="n"), "is not counter"),
    (dict(name="f", type="counter", labels=["Interfaces"], flatten=["Interfaces"]), "flatten"),
    (dict(name="v", type="counter", valueKey="DnsLatencyMs"), "value key 'DnsLatencyMs'"),
    (dict(name="l", type="counter", labels=["SrcK8S_Namespace", "Dscp"]), "key 'Dscp' is outside the dimension list"),
    (dict(name="k", type="counter", filters=[dict(key="DnsFlagsResponseCode", value="NoError", type="equal")]), "key 'DnsFlagsResponseCode' is outside"),
    (dict(name="i", type="counter", filters=[dict(key="Proto", value="$(Bytes)", type="equal")]), "key 'Bytes' is outside"),
    (dict(name="a", type="counter", labels=["SrcAddr"]), "key 'SrcAddr' is outside"),
])
def test_items_this_path_cannot_serve(nf, item, message):
    with pytest.raises(ValueError) as e:
        nf.PromCounters([item])
    assert message in str(e.value)


def test_more_than_eight_groupings(nf):
    keys = ["SrcK8S_" + s for s in nf.metrics.K8S_SUFFIXES]
    nf.PromCounters([dict(name="m%d" % k, type="counter", labels=[key]) for k, key in enumerate(keys[:8])])
    with pytest.raises(ValueError) as e:
        nf.PromCounters([dict(name="m%d" % k, type="counter", labels=[key]) for k, key in enumerate(keys)])
    assert "9 distinct groupings" in str(e.value)


def test_grouping_is_labels_and_filters_and_variables_and_is_shared(nf):
    L = nf._lib
    items = [
        dict(name="a", type="counter", labels=["SrcK8S_Namespace", "DstK8S_Namespace"]),
        dict(name="b", type="counter", valueKey="Bytes", labels=["DstK8S_Namespace"], filters=[dict(key="SrcK8S_Namespace", type="presence")]),     # the same keys
        dict(name="c", type="counter", labels=["Proto"], filters=[dict(key="K8S_FlowLayer", value="app"), dict(key="FlowDirection", value="$(Proto)", type="not_equal")]),
        dict(name="d", type="counter", filters=[dict(key="SrcK8S_HostIP", value="$(DstK8S_HostIP)", type="equal"), dict(key="SrcK8S_Zone", value="$(DstK8S_Zone)", type="match_regex")]),
        dict(name="e", type="counter"),
        dict(name="f", type="counter", labels=["SrcSubnetLabel", "DstSubnetLabel", "SrcK8S_Type", "DstK8S_OwnerType", "DstK8S_OwnerName", "SrcK8S_NetworkName", "DstK8S_HostName", "SrcK8S_Name"]),
    ]
    p = nf.PromCounters(items)
    ns = L.DIM_SRC_K8S(0) | L.DIM_DST_K8S(0)
    assert p.groupings == [ns, L.DIM_PROTO | L.DIM_FLOW_LAYER | L.DIM_FLOW_DIRECTION,
                           L.DIM_SRC_K8S(6) | L.DIM_DST_K8S(6) | L.DIM_SRC_K8S(8),           # a regex's value is no variable: DstK8S_Zone is not read
                           0, L.DIM_SRC_SUBNET_LABEL | L.DIM_DST_SUBNET_LABEL | L.DIM_SRC_K8S(2) | L.DIM_DST_K8S(4) | L.DIM_DST_K8S(3) | L.DIM_SRC_K8S(5) |
                           L.DIM_DST_K8S(7) | L.DIM_SRC_K8S(1)]
    assert [it["grouping"] for it in p.items] == [0, 0, 1, 2, 3, 4]
    assert L.DIM_ALL == (1 << 23) - 1 and set(nf.metrics.KEY_DIMS.values()) == {1 << b for b in range(23)}


# ---- the per-group evaluation against the restatement
ENTRIES = [
    ("10.0.0.1", dict(namespace="shop", name="cart", kind="Pod", owner_name="cart", owner_kind="Deployment", network_name="primary", host_ip="192.168.0.1", host_name="n1", zone="z1")),
    ("10.0.0.2", dict(namespace="shop", name="pay", kind="Pod", owner_name="pay", owner_kind="Deployment", network_name="primary", host_ip="192.168.0.2", host_name="n2", zone="")),
    ("10.0.0.3", dict(namespace="openshift-dns", name="dns", kind="Pod", host_ip="192.168.0.1")),
    ("10.0.0.4", dict(name="n1", kind="Node", host_ip="192.168.0.1", host_name="ignored-without", zone="z1")),
    ("10.0.0.5", dict(namespace="shop", name="orphan", kind="Pod", host_name="no-host-ip")),
    ("10.0.0.6", dict(namespace=b"q\"b\\\xff", name="cart", kind="Service")),
]
LABELS = [b"internal", b"", b"ext \xc3\xa9"]
ITEMS = [
    dict(name="flows", type="counter", labels=["SrcK8S_Namespace", "DstK8S_Namespace", "K8S_FlowLayer"], remap={"K8S_FlowLayer": "layer"}),
    dict(name="bytes", type="counter", valueKey="Bytes", labels=["SrcK8S_Namespace", "DstK8S_Namespace"], filters=[dict(key="K8S_FlowLayer", value="app", type="equal")]),
    dict(name="kpackets", type="counter", valueKey="Packets", valueScale=1000, labels=["SrcSubnetLabel", "DstSubnetLabel", "Proto"],
         filters=[dict(key="Proto", value="^(6|17)$", type="match_regex"), dict(key="SrcSubnetLabel", type="presence")]),
    dict(name="zones", type="counter", labels=["SrcK8S_Zone", "SrcK8S_HostName", "DstK8S_HostIP", "FlowDirection"],
         filters=[dict(key="DstK8S_Zone", type="absence"), dict(key="FlowDirection", value="2", type="not_equal"), dict(key="SrcK8S_HostName", value="^$", type="not_match_regex")]),
    dict(name="same_node", type="counter", filters=[dict(key="SrcK8S_HostIP", value="$(DstK8S_HostIP)", type="equal")]),
]


def enriched(src, dst, label=(None, None), direction=None, layer=None, proto=None, bytes_=0, packets=0) -> dict:
    """What the stage's rules leave of one flow, for the keys of the dimension list: src / dst index ENTRIES (None: no row)."""
    m = {}
    for row, prefix in ((src, "SrcK8S_"), (dst, "DstK8S_")):
        if row is None:
            continue
        info = ENTRIES[row][1]
        g = lambda f: M._b(info.get(f) or b"")  # noqa: E731
        if g("namespace"):
            m[prefix + "Namespace"] = g("namespace")
        for f, s in (("name", "Name"), ("kind", "Type"), ("owner_name", "OwnerName"), ("owner_kind", "OwnerType"), ("network_name", "NetworkName")):
            m[prefix + s] = g(f)
        if g("host_ip"):
            m[prefix + "HostIP"] = g("host_ip")
            if g("host_name"):
                m[prefix + "HostName"] = g("host_name")
        if info.get("zone") is not None:
            m[prefix + "Zone"] = g("zone")
    for k, key in zip(label, ("SrcSubnetLabel", "DstSubnetLabel")):
        if k is not None and LABELS[k]:
            m[key] = LABELS[k]
    if direction is not None:
        m["FlowDirection"] = direction
    if layer is not None:
        m["K8S_FlowLayer"] = layer
    if proto is not None:
        m["Proto"] = proto
    if bytes_:
        m["Bytes"] = bytes_
    if packets:
        m["Packets"] = packets
    return {k.encode(): v for k, v in m.items()}


def hand_groups(nf, met, dims, flows):
    """The groups a fold of `flows` would return for one grouping, built in plain Python from the metrics table's classes."""
    L = nf._lib
    g = met.groupings.index(dims)

    def side_keys(side, row):                                           # the selected keys of one side of a flow whose row is `row`
        return nf.metrics.group_keys(dims & (0x1FF << (9 * side)), {"src_class": 1, "dst_class": 1}, ENTRIES, LABELS, lambda *_: row, g)

    def cls(side, row):                                                 # the class whose first row carries this row's selected keys
        if row is None or not (dims >> (9 * side)) & 0x1FF:
            return 0
        hits = [c for c in range(1, met.n_classes(g, side) + 1) if side_keys(side, met.class_row(g, side, c)) == side_keys(side, row)]
        assert len(hits) == 1, (side, row, hits)
        return hits[0]

    acc = {}
    for f in flows:
        key = (cls(0, f["src"]), cls(1, f["dst"]),
               f["label"][0] if dims & L.DIM_SRC_SUBNET_LABEL and f["label"][0] is not None else L.NET_NO_LABEL,
               f["label"][1] if dims & L.DIM_DST_SUBNET_LABEL and f["label"][1] is not None else L.NET_NO_LABEL,
               f["direction"] if dims & L.DIM_FLOW_DIRECTION and f["direction"] is not None else L.NET_NO_DIRECTION,
               {None: 0, b"infra": 1, b"app": 2}[f["layer"]] if dims & L.DIM_FLOW_LAYER else 0,
               f["proto"] if dims & L.DIM_PROTO and f["proto"] is not None else 0, 1 if dims & L.DIM_PROTO and f["proto"] is not None else 0)
        s = acc.setdefault(key, [0, 0, 0, 0, 0])
        for k, v in enumerate((1, f["bytes_"], f["packets"], int(f["bytes_"] != 0), int(f["packets"] != 0))):
            s[k] += v
    out = np.zeros(len(acc), dtype=nf.METRIC_GROUP)
    for k, (key, s) in enumerate(acc.items()):
        out[k] = key + tuple(s) + (0,)
    return out


def test_group_evaluation_against_the_restatement(nf):
    rng = np.random.default_rng(5)
    flows = []
    for _ in range(400):
        pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
        flows.append(dict(src=pick([None, 0, 1, 2, 3, 4, 5]), dst=pick([None, 0, 1, 2, 3, 4, 5]), label=(pick([None, 0, 1, 2]), pick([None, 0, 1, 2])),
                          direction=pick([None, 0, 1, 2]), layer=pick([b"app", b"infra"]), proto=pick([None, 6, 17, 1, 60]),
                          bytes_=pick([0, 1, 1500, 2**40]), packets=pick([0, 1, 7, 2**32 - 1])))
    ref = M.Counters(ITEMS, prefix="netobserv_")
    for f in flows:
        ref.encode(enriched(**f))
    p = nf.PromCounters(ITEMS, prefix="netobserv_")
    with nf.K8sTable(ENTRIES) as k8s, nf.MetricsTable(k8s, p.groupings) as met:
        p.add_groups([hand_groups(nf, met, d, flows) for d in p.groupings], ENTRIES, LABELS, met.class_row)
    assert set(p.values) == set(ref.values) and len(p.values) > 40
    for name in ("flows", "bytes", "kpackets", "zones", "same_node"):
        assert series(p.values, "netobserv_" + name), name
    for key, v in ref.values.items():
        assert abs(p.values[key] - v) <= len(flows) * 2.0**-52 * abs(v), key               # n rounded additions against one rounding of the sum
        if key[0] in ("netobserv_flows", "netobserv_zones", "netobserv_same_node"):
            assert p.values[key] == v                                                      # small integers: exact


def test_a_group_without_the_value_key_registers_no_series(nf):
    p = nf.PromCounters([dict(name="b", type="counter", valueKey="Bytes", labels=["Proto"]), dict(name="p", type="counter", valueKey="Packets", labels=["Proto"]),
                         dict(name="f", type="counter", labels=["Proto"])])
    groups = np.zeros(2, dtype=nf.METRIC_GROUP)
    groups["src_label"] = groups["dst_label"] = nf._lib.NET_NO_LABEL
    groups["direction"] = nf._lib.NET_NO_DIRECTION
    groups[0]["proto"], groups[0]["is_ip"], groups[0]["flows"], groups[0]["packets"], groups[0]["flows_with_packets"] = 6, 1, 3, 9, 2
    groups[1]["flows"], groups[1]["bytes"], groups[1]["flows_with_bytes"] = 2, 2**60, 1
    p.add_groups([groups], [], [], None)
    assert p.values == {("b", (("Proto", b""),)): float(2**60), ("p", (("Proto", b"6"),)): 9.0, ("f", (("Proto", b"6"),)): 3.0, ("f", (("Proto", b""),)): 2.0}


# ---- the host side from plain C, and the ABI
def test_metrics_host_check_compiles_and_runs(nf, tmp_path):
    lib_dir = os.path.dirname(nf._lib.LIB_PATH)
    exe = str(tmp_path / "metrics_host_check")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "c", "metrics_host_check.c"),
                           "-o", exe, "-L", lib_dir, "-lnfagg", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "metrics host check ok", out.stderr


def test_symbols_layout_and_host_only_tables(nf):
    L = nf._lib
    for name in ("nfagg_metrics_table_create", "nfagg_metrics_table_destroy", "nfagg_metrics_n_classes", "nfagg_metrics_class_row", "nfagg_metrics_fold",
                 "nfagg_metrics_fold_device"):
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    g = nf.METRIC_GROUP
    assert g.itemsize == 64 and [g.fields[f][1] for f in g.names] == [0, 4, 8, 10, 12, 13, 14, 15, 16, 24, 32, 40, 48, 56]
    assert (L.MET_MAX_GROUPINGS, L.MET_MAX_GROUPS) == (8, 1 << 20)
    with nf.K8sTable(ENTRIES) as k8s:
        with nf.MetricsTable(k8s, [L.DIM_SRC_K8S(0), L.DIM_DST_K8S(8) | L.DIM_PROTO]) as met:
            assert (met.n_classes(0, 0), met.n_classes(0, 1), met.n_classes(1, 0), met.n_classes(1, 1)) == (4, 0, 0, 3)
            assert met.class_row(0, 0, 0) == L.K8S_NO_ROW and [met.class_row(0, 0, c) for c in (1, 2, 3, 4)] == [0, 2, 3, 5]
            assert [met.class_row(1, 1, c) for c in (1, 2, 3)] == [0, 1, 2]                # "z1", "" and no zone
            with pytest.raises(nf.NfaggError) as e:
                met.class_row(0, 0, 5)
            assert e.value.code == L.EINVAL and "class 5 of 4" in str(e.value)
        for bad, message in (([1 << 23], "unknown dimension bits"), ([], "0 groupings"), ([0] * 9, "9 groupings")):
            with pytest.raises(nf.NfaggError) as e:
                nf.MetricsTable(k8s, bad)
            assert e.value.code == L.EINVAL and message in str(e.value)


def test_exporters_want_k8s_with_metrics(nf):
    p = nf.PromCounters([dict(name="f", type="counter")])
    with pytest.raises(ValueError):
        nf.DirectFLPJSON(None, None, metrics=p)
    with pytest.raises(ValueError):
        nf.MapTracer(None, 0, 0).evictFlowsJSON(metrics=p)
