"""Content flow metrics (histograms, the RTT / DNS / drop values and labels), CPU side: PromMetrics' integer thresholds against a
brute-force float comparison; its validation errors and grouping derivation; its per-group evaluation, fed with hand-built
nfagg_metric_group_content arrays, against the per-flow restatement of tests/flp_metrics_content_ref.py; the host-only spec
validation and its messages; nfagg_flp_enum_name against the names of tests/flp_json_content_ref.py; tools/c/metrics_content_host_check.c
compiled with -fsanitize=address,undefined and run (a stand-alone program: no sanitizer touches code loaded into python); and what
must not have moved: DIM_ALL, KEY_DIMS, PromCounters' refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_content_ref as C  # noqa: E402
import flp_metrics_content_ref as H  # noqa: E402
import flp_metrics_ref as M  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
I64_MIN, I64_MAX = -2**63, 2**63 - 1
CUSTOM = [-2.5, -1e-3, 0.0, 0.3, 1.0, 7.0, 1e3, 123456.789, 2.0**40, 9.3e18]


# ---- integer thresholds
def observed(x: int, scale: float) -> float:
    """The float the reference buckets for the integer x (ConvertToFloat64, / ValueScale unless 0), written out here again."""
    return float(x) / scale if scale != 0 else float(x)


@pytest.mark.parametrize("scale", [0, 1, 3, 1000, 1e9])
@pytest.mark.parametrize("bounds", [H.DEF_BUCKETS, CUSTOM], ids=["DefBuckets", "custom"])
def test_thresholds_against_the_float_comparison(nf, scale, bounds):
    """For every x within 50 of a threshold (and of +-bound * scale, where a wrong threshold would sit) and at the domain's ends,
    x <= threshold says what observed(x) <= bound says. Both signs: the RTT domain is all of int64."""
    T = nf.metrics.threshold
    for lo, hi in ((I64_MIN, I64_MAX), (0, 0xFFFF), (-(2**63 // 10**6), (2**63 - 1) // 10**6)):
        ts = [T(b, scale, lo, hi) for b in bounds]
        assert [t for t in ts if t is not None] == sorted(t for t in ts if t is not None)          # non-decreasing, as the ABI asks
        for b, t in zip(bounds, ts):
            near = {lo, hi, 0, -1, 1}
            for c in ([t] if t is not None else []) + [int(b * (scale or 1)), -int(b * (scale or 1))]:
                near.update(range(c - 50, c + 51))
            for x in near:
                if lo <= x <= hi:
                    assert (t is not None and x <= t) == (observed(x, scale) <= b), (b, scale, x, t)
    if scale == 1:
        assert [T(b, 1, 0, 0xFFFF) for b in H.DEF_BUCKETS] == [0, 0, 0, 0, 0, 0, 0, 1, 2, 5, 10]   # seven equal thresholds
    if scale == 1e9:
        assert T(.005, 1e9, I64_MIN, I64_MAX) == 5_000_000 and T(10, 1e9, I64_MIN, I64_MAX) == 10_000_000_000


def test_a_bound_below_the_domain(nf):
    T = nf.metrics.threshold
    assert T(-1.0, 0, 0, 0xFFFF) is None and T(-0.5, 1000, 0, 2**64 - 1) is None and T(0.0, 0, 0, 0xFFFF) == 0
    assert T(1e30, 0, I64_MIN, I64_MAX) == I64_MAX and T(-1e30, 0, I64_MIN, I64_MAX) is None
    # the leading bounds take no flow: the device gets the rest, the result keeps every bucket
    p = nf.PromMetrics([dict(name="h", type="histogram", valueKey="PktDropBytes", buckets=[-5, -1, 10, 100])], item_buckets=True)
    assert p.specs()[0]["bounds"] == (10, 100) and p.items[0]["skip"] == 2
    g = np.zeros(2, dtype=nf.METRIC_GROUP_CONTENT)
    g["bucket"], g["flows"], g["flows_with_value"][:, 0], g["value_sum"][:, 0] = [0, 2], 3, 3, [12, 900]
    p.add_groups([g], [], [], None)
    assert p.histograms == {("h", ()): dict(buckets=[0, 0, 3, 0, 3], count=6, sum=912.0)}
    # every bound below: one threshold nothing reaches, everything in +Inf
    q = nf.PromMetrics([dict(name="h", type="histogram", valueKey="PktDropPackets", buckets=[-5, -1])], item_buckets=True)
    assert q.specs()[0]["bounds"] == (I64_MIN,)
    g = np.zeros(1, dtype=nf.METRIC_GROUP_CONTENT)
    g["bucket"], g["flows"], g["flows_with_value"][:, 0], g["value_sum"][:, 0] = 1, 4, 4, 8
    q.add_groups([g], [], [], None)
    assert q.histograms == {("h", ()): dict(buckets=[0, 0, 4], count=4, sum=8.0)}


# ---- validation
@pytest.mark.parametrize("item, message", [
    (dict(name="g", type="gauge", valueKey="Bytes"), "neither counter nor histogram"),
    (dict(name="a", type="agg_histogram", valueKey="Bytes"), "neither counter nor histogram"),
    (dict(name="n"), "neither counter nor histogram"),
    (dict(name="f", type="counter", labels=["Interfaces"], flatten=["Interfaces"]), "flatten"),
    (dict(name="v", type="counter", valueKey="DnsErrno"), "value key 'DnsErrno'"),
    (dict(name="l", type="counter", labels=["SrcK8S_Namespace", "Dscp"]), "key 'Dscp' is outside the dimension lists"),
    (dict(name="d", type="counter", labels=["DnsId"]), "key 'DnsId' is outside"),
    (dict(name="e", type="counter", filters=[dict(key="DnsId", value="7", type="equal")]), "key 'DnsId' serves presence and absence filters only"),
    (dict(name="o", type="histogram", valueKey="TimeFlowRttNs", filters=[dict(key="TimeFlowRttNs", value="^1", type="match_regex")]), "serves presence and absence"),
    (dict(name="p", type="counter", filters=[dict(key="TimeFlowRttNs", type="presence")]), "key 'TimeFlowRttNs' is outside"),
    (dict(name="i", type="counter", filters=[dict(key="Proto", value="$(PktDropBytes)", type="equal")]), "key 'PktDropBytes' is outside"),
    (dict(name="h", type="histogram"), "a histogram needs a value key"),
    (dict(name="s", type="histogram", valueKey="Bytes", valueScale=-1), "negative valueScale"),
])
def test_items_this_path_cannot_serve(nf, item, message):
    with pytest.raises(ValueError) as e:
        nf.PromMetrics([item])
    assert message in str(e.value)


def test_bucket_errors(nf):
    for buckets, message in (([1, 1], "buckets must increase"), ([3, 2], "buckets must increase"), (list(range(33)), "33 buckets, more than 32"),
                             ([1e19], "passes INT64_MAX"), ([-3, -2], None)):
        item = dict(name="b", type="histogram", valueKey="Bytes", buckets=buckets)
        nf.PromMetrics([item])                                             # the vendored FLP ignores the item's buckets: DefBuckets
        if message is None:
            nf.PromMetrics([item], item_buckets=True)
            continue
        with pytest.raises(ValueError) as e:
            nf.PromMetrics([item], item_buckets=True)
        assert message in str(e.value)
    with pytest.raises(ValueError) as e:                                   # int64 has no integer below such bounds, and INT64_MIN is a value
        nf.PromMetrics([dict(name="r", type="histogram", valueKey="TimeFlowRttNs", buckets=[-1e30])], item_buckets=True)
    assert "below the value's domain" in str(e.value)
    assert nf.PromMetrics([dict(name="r", type="histogram", valueKey="TimeFlowRttNs")]).items[0]["bounds"] == tuple(H.DEF_BUCKETS)


def test_more_than_eight_groupings(nf):
    keys = ["SrcK8S_" + s for s in nf.metrics.K8S_SUFFIXES]
    nf.PromMetrics([dict(name="m%d" % k, type="histogram", valueKey="TimeFlowRttNs", labels=[key]) for k, key in enumerate(keys[:8])])
    with pytest.raises(ValueError) as e:
        nf.PromMetrics([dict(name="m%d" % k, type="histogram", valueKey="TimeFlowRttNs", labels=[key]) for k, key in enumerate(keys)])
    assert "9 distinct groupings" in str(e.value)


def test_groupings_are_shared_where_they_can_be(nf):
    L = nf._lib
    ns = ["SrcK8S_Namespace", "DstK8S_Namespace"]
    drop = ["PktDropLatestState", "PktDropLatestDropCause"]
    p = nf.PromMetrics([
        dict(name="rtt", type="histogram", valueKey="TimeFlowRttNs", valueScale=1e9, labels=ns),
        dict(name="flows", type="counter", labels=ns),                                           # joins the histogram's grouping: it sums over the buckets
        dict(name="bytes", type="counter", valueKey="Bytes", labels=ns),
        dict(name="rtt_sum", type="counter", valueKey="TimeFlowRttNs", labels=ns),               # the histogram's slot
        dict(name="dns", type="histogram", valueKey="DnsLatencyMs", valueScale=1000, labels=ns + ["DnsFlagsResponseCode"]),
        dict(name="dns_ms", type="histogram", valueKey="DnsLatencyMs", labels=ns + ["DnsFlagsResponseCode"]),    # other thresholds: its own grouping
        dict(name="drop_bytes", type="counter", valueKey="PktDropBytes", labels=ns + drop),
        dict(name="drop_packets", type="counter", valueKey="PktDropPackets", labels=ns + drop),  # the second slot
        dict(name="drop_rtt", type="counter", valueKey="TimeFlowRttNs", labels=ns + drop),       # no third slot: a grouping of its own
        dict(name="with_dns", type="counter", labels=ns, filters=[dict(key="DnsId", type="presence")]),      # DnsId is the response code's "none": the dns grouping
        dict(name="ipsec", type="counter", labels=["IPSecStatus"], filters=[dict(key="IPSecStatus", type="presence")]),
    ])
    nsd = L.DIM_SRC_K8S(0) | L.DIM_DST_K8S(0)
    assert [it["grouping"] for it in p.items] == [0, 0, 0, 0, 1, 2, 3, 3, 4, 1, 5]
    specs = p.specs()
    assert [(s["dims"], s["xdims"], s["value"], s["hist"], len(s["bounds"])) for s in specs] == [
        (nsd, 0, (L.MET_VALUE_RTT_NS,), 1, 11), (nsd, L.XDIM_DNS_RCODE, (L.MET_VALUE_DNS_LATENCY_MS,), 1, 11),
        (nsd, L.XDIM_DNS_RCODE, (L.MET_VALUE_DNS_LATENCY_MS,), 1, 11),
        (nsd, L.XDIM_DROP_CAUSE | L.XDIM_DROP_STATE, (L.MET_VALUE_DROP_BYTES, L.MET_VALUE_DROP_PACKETS), 0, 0),
        (nsd, L.XDIM_DROP_CAUSE | L.XDIM_DROP_STATE, (L.MET_VALUE_RTT_NS,), 0, 0), (0, L.XDIM_IPSEC_STATUS, (), 0, 0)]
    assert specs[1]["bounds"] == (5, 10, 25, 50, 100, 250, 500, 1000, 2500, 5000, 10000) and specs[2]["bounds"] == (0, 0, 0, 0, 0, 0, 0, 1, 2, 5, 10)
    assert [it["slot"] for it in p.items] == [0, None, None, 0, 0, 0, 0, 1, 0, None, None]
    with nf.K8sTable([]) as k8s, nf.MetricsTable(k8s, None, specs=specs) as met:               # the library accepts what PromMetrics derives
        assert met.groupings == [nsd] * 5 + [0]
    # presence of the own value key filters nothing; absence alone leaves no series; both ORed: presence wins
    q = nf.PromMetrics([dict(name="a", type="counter", valueKey="PktDropBytes", filters=[dict(key="PktDropBytes", type="presence")]),
                        dict(name="b", type="counter", valueKey="PktDropBytes", filters=[dict(key="PktDropBytes", type="absence")]),
                        dict(name="c", type="counter", valueKey="PktDropBytes", filters=[dict(key="PktDropBytes", type="absence"), dict(key="PktDropBytes", type="presence")])])
    assert [it["dead"] for it in q.items] == [False, True, False] and len(q.groupings) == 1
    g = np.zeros(1, dtype=nf.METRIC_GROUP_CONTENT)
    g["bucket"], g["flows"], g["flows_with_value"][:, 0], g["value_sum"][:, 0] = 0xFF, 5, 2, 3000
    q.add_groups([g], [], [], None)
    assert q.values == {("a", ()): 3000.0, ("c", ()): 3000.0}


# ---- per-group evaluation against the per-flow restatement
ITEMS = [
    dict(name="rtt_seconds", type="histogram", valueKey="TimeFlowRttNs", valueScale=1e9, labels=["Proto"]),
    dict(name="dns_latency_seconds", type="histogram", valueKey="DnsLatencyMs", valueScale=1000, labels=["DnsFlagsResponseCode"],
         filters=[dict(key="DnsId", type="presence")]),
    dict(name="dns_latency_ms", type="histogram", valueKey="DnsLatencyMs", labels=["Proto"], buckets=[-10, 0, 3, 700]),
    dict(name="drop_bytes_total", type="counter", valueKey="PktDropBytes", labels=["PktDropLatestState", "PktDropLatestDropCause"]),
    dict(name="drop_packets_total", type="counter", valueKey="PktDropPackets", labels=["PktDropLatestState", "PktDropLatestDropCause"],
         filters=[dict(key="PktDropLatestDropCause", value="^SKB_", type="match_regex")]),
    dict(name="ipsec_flows_total", type="counter", labels=["IPSecStatus"], filters=[dict(key="IPSecStatus", type="presence")]),
    dict(name="no_dns_bytes_total", type="counter", valueKey="Bytes", labels=["Proto"], filters=[dict(key="DnsId", type="absence")]),
    dict(name="bytes_hist", type="histogram", valueKey="Bytes", valueScale=3, labels=["IPSecStatus"]),
    dict(name="rtt_total", type="counter", valueKey="TimeFlowRttNs", labels=["Proto"], filters=[dict(key="TimeFlowRttNs", type="presence")]),
    dict(name="latency_by_code", type="counter", valueKey="DnsLatencyMs", labels=["DnsFlagsResponseCode"]),       # ServFail: negative latencies only
]


def make_flows(rng, n):
    """The RTT stays at 2^50 and below: a group's sum is a 64-bit integer (modulo 2^64, include/nfagg.h), which 600 flows of 2^62
    would wrap where the reference's floats do not; 2^50 still takes the sums past 2^53, where a float addition rounds."""
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    flows = []
    for _ in range(n):
        flows.append(dict(proto=pick([None, 6, 17]), bytes_=pick([0, 1, 2, 3, 14, 15, 16, 31, 1500, 2**40]),
                          rtt=pick([None, None, -3, 1, 4_999_999, 5_000_000, 5_000_001, 10**10, 10**10 + 1, 2**50]),
                          dns=pick([None, None, (0, -1), (3, 0), (3, 5), (3, 6), (0, 700), (15, 701), (11, -10), (2, -11), (0, 10**7)]),
                          drop=pick([None, None, (2, 1, 0, 0), (2, 1, 100, 3), ((1 << 24) + 4, 0, 65535, 65535), (77, 200, 1, 1), (999, 12, 5, 5)]),
                          ipsec=pick([0, 0, 1, 2])))
    return flows


def flow_map(f) -> dict:
    """The keys RecordToMap writes for one hand-made flow, with the names of flp_json_content_ref."""
    m = {}
    if f["proto"] is not None:
        m[b"Proto"] = f["proto"]
    if f["bytes_"]:
        m[b"Bytes"] = f["bytes_"]
    if f["rtt"] is not None:
        m[b"TimeFlowRttNs"] = f["rtt"]
    if f["dns"] is not None:
        m[b"DnsId"], m[b"DnsFlagsResponseCode"], m[b"DnsLatencyMs"] = 7, C.dns_rcode(f["dns"][0]), f["dns"][1]
    if f["drop"] is not None:
        cause, state, nbytes, packets = f["drop"]
        m[b"PktDropLatestDropCause"], m[b"PktDropLatestState"], m[b"PktDropBytes"], m[b"PktDropPackets"] = C.drop_cause(cause), C.tcp_state(state), nbytes, packets
    if f["ipsec"]:
        m[b"IPSecStatus"] = b"success" if f["ipsec"] == 1 else b"error"
    return m


def hand_groups(nf, spec, flows):
    """The groups nfagg_metrics_fold_content would return for one spec without Kubernetes or net dimensions, in plain Python."""
    L = nf._lib
    src = {L.MET_VALUE_RTT_NS: lambda f: f["rtt"], L.MET_VALUE_DNS_LATENCY_MS: lambda f: f["dns"][1] if f["dns"] else None,
           L.MET_VALUE_DROP_BYTES: lambda f: f["drop"][2] if f["drop"] else None, L.MET_VALUE_DROP_PACKETS: lambda f: f["drop"][3] if f["drop"] else None,
           L.MET_VALUE_BYTES: lambda f: f["bytes_"] or None}
    acc = {}
    for f in flows:
        vals = [src[s](f) for s in spec["value"]]
        bucket = L.MET_NO_BUCKET
        if spec["hist"] and vals[spec["hist"] - 1] is not None:
            bucket = next((k for k, b in enumerate(spec["bounds"]) if vals[spec["hist"] - 1] <= b), len(spec["bounds"]))
        xd = spec["xdims"]
        key = (f["proto"] or 0 if spec["dims"] & L.DIM_PROTO else 0, int(f["proto"] is not None) if spec["dims"] & L.DIM_PROTO else 0,
               f["drop"][0] if xd & L.XDIM_DROP_CAUSE and f["drop"] else 0, f["drop"][1] if xd & L.XDIM_DROP_STATE and f["drop"] else 0xFFFF,
               f["dns"][0] if xd & L.XDIM_DNS_RCODE and f["dns"] else 0xFF, f["ipsec"] if xd & L.XDIM_IPSEC_STATUS else 0, bucket)
        s = acc.setdefault(key, [0] * 9)
        add = [1, f["bytes_"], 0, int(f["bytes_"] != 0), 0] + [v or 0 for v in vals] + [0] * (2 - len(vals)) + [int(v is not None) for v in vals] + [0] * (2 - len(vals))
        for k, v in enumerate(add):
            s[k] += v
    out = np.zeros(len(acc), dtype=nf.METRIC_GROUP_CONTENT)
    out["src_label"] = out["dst_label"] = L.NET_NO_LABEL
    out["direction"] = L.NET_NO_DIRECTION
    for k, (key, s) in enumerate(acc.items()):
        out[k]["proto"], out[k]["is_ip"], out[k]["drop_cause"], out[k]["drop_state"], out[k]["dns_rcode"], out[k]["ipsec_status"], out[k]["bucket"] = key
        out[k]["flows"], out[k]["bytes"], out[k]["packets"], out[k]["flows_with_bytes"], out[k]["flows_with_packets"] = s[:5]
        out[k]["value_sum"] = [v % 2**64 for v in s[5:7]]
        out[k]["flows_with_value"] = s[7:9]
    return out


def test_group_evaluation_against_the_restatement(nf):
    flows = make_flows(np.random.default_rng(7), 600)
    maps = [flow_map(f) for f in flows]
    counters = M.Counters([it for it in ITEMS if it["type"] == "counter"], prefix="netobserv_")
    hists = H.Histograms([it for it in ITEMS if it["type"] == "histogram"], prefix="netobserv_", item_buckets=True)
    for m in maps:
        counters.encode(m)
        hists.encode(m)
    p = nf.PromMetrics(ITEMS, prefix="netobserv_", item_buckets=True)
    for _ in range(2):                                                     # a second call doubles everything
        p.add_groups([hand_groups(nf, sp, flows) for sp in p.specs()], [], [], None)
    assert set(p.values) == set(counters.values) and len(p.values) > 12 and set(p.histograms) == set(hists.values) and len(p.histograms) > 12
    scale = {"netobserv_" + it["name"]: it.get("valueScale", 0) for it in ITEMS}
    exact = H.exact_sums(maps, ITEMS, "netobserv_")
    for key, v in counters.values.items():
        assert p.values[key] == 2 * (float(exact[key]) / scale[key[0]] if scale[key[0]] else float(exact[key])), key
        assert abs(p.values[key] - 2 * v) <= len(flows) * 2.0**-52 * abs(2 * v), key
    for key, h in hists.values.items():
        got = p.histograms[key]
        assert got["buckets"] == [2 * b for b in h["buckets"]] and got["count"] == 2 * h["count"] == sum(got["buckets"]), key
        assert got["sum"] == 2 * (float(exact[key]) / scale[key[0]] if scale[key[0]] else float(exact[key])), key      # one rounding of the exact integer sum
        assert abs(got["sum"] - 2 * h["sum"]) <= len(flows) * 2.0**-52 * abs(2 * h["sum"]), key
    for name in ("rtt_seconds", "dns_latency_seconds", "dns_latency_ms", "bytes_hist"):
        mine = [h for (n, _), h in hists.values.items() if n == "netobserv_" + name]
        assert mine and sum(1 for k in range(len(mine[0]["buckets"])) if any(h["buckets"][k] for h in mine)) >= 3, name   # several buckets are hit
    assert any(h["buckets"][0] > 0 for (n, _), h in p.histograms.items() if n == "netobserv_dns_latency_ms")      # negative values have a bucket
    assert p.values[("netobserv_latency_by_code", (("DnsFlagsResponseCode", b"ServFail"),))] < 0                   # and a two's complement sum a sign
    assert {dict(l)["PktDropLatestDropCause"] for n, l in p.values if n == "netobserv_drop_bytes_total"} == {
        b"SKB_DROP_REASON_NOT_SPECIFIED", b"NetworkEvent_NetworkPolicy", C.drop_cause(77), b"SKB_DROP_UNKNOWN_CAUSE"}


# ---- the library's host side
def test_spec_validation_messages(nf):
    L = nf._lib
    ok = dict(dims=L.DIM_PROTO, xdims=L.XDIM_ALL, value=(L.MET_VALUE_RTT_NS, L.MET_VALUE_BYTES), hist=2, bounds=[I64_MIN, 0, 0, I64_MAX])
    with nf.K8sTable([]) as k8s:
        with nf.MetricsTable(k8s, None, specs=[ok] * 8) as met:
            assert met.groupings == [L.DIM_PROTO] * 8
        for bad, message in ((dict(dims=1 << 23), "grouping 1: unknown dimension bits 0x800000"), (dict(xdims=16), "grouping 1: unknown xdims bits 0x10"),
                             (dict(value=(7,)), "grouping 1: value[0]: unknown source 7"), (dict(value=(0, 9)), "grouping 1: value[1]: unknown source 9"),
                             (dict(value=(1,), hist=2, bounds=[1]), "grouping 1: hist 2 names the empty value[1]"), (dict(hist=1, bounds=[1]), "hist 1 names the empty value[0]"),
                             (dict(value=(1,), hist=3, bounds=[1]), "grouping 1: hist 3"), (dict(value=(1,), hist=1), "grouping 1: n_bounds 0, not 1..32"),
                             (dict(value=(1,), hist=1, bounds=range(33), n_bounds=33), "grouping 1: n_bounds 33, not 1..32"),
                             (dict(value=(1,), hist=1, bounds=[0, 5, 4]), "grouping 1: bounds[2] is below bounds[1]"),
                             (dict(struct_size=272), "grouping 1: struct_size 272, not 280")):
            with pytest.raises(nf.NfaggError) as e:
                nf.MetricsTable(k8s, None, specs=[ok, bad])
            assert e.value.code == L.EINVAL and message in str(e.value), message
        for n in (0, 9):
            with pytest.raises(nf.NfaggError) as e:
                nf.MetricsTable(k8s, None, specs=[ok] * n)
            assert e.value.code == L.EINVAL and "%d groupings" % n in str(e.value)


def test_enum_names_against_the_restatement(nf):
    L = nf._lib
    for r in range(16):
        assert nf.flp_enum_name(L.FLP_ENUM_DNS_RCODE, r) == C.dns_rcode(r)
    for st in list(range(14)) + [200, 255]:
        assert nf.flp_enum_name(L.FLP_ENUM_TCP_STATE, st) == C.tcp_state(st)
    causes = list(range(0, 90)) + [(3 << 16) + k for k in range(0, 14)] + [(1 << 24) + k for k in range(0, 12)] + [12345, 2**31, 2**32 - 1]
    for c in causes:
        assert nf.flp_enum_name(L.FLP_ENUM_DROP_CAUSE, c) == C.drop_cause(c), c
    assert nf.flp_enum_name(L.FLP_ENUM_DROP_CAUSE, 12345) == b"SKB_DROP_UNKNOWN_CAUSE" and nf.flp_enum_name(L.FLP_ENUM_DROP_CAUSE, (1 << 24) + 4) == b"NetworkEvent_NetworkPolicy"
    with pytest.raises(nf.NfaggError):
        nf.flp_enum_name(3, 0)


def test_the_content_hash_reads_the_key_fields(nf):
    g = np.zeros(3, dtype=nf.METRIC_GROUP_CONTENT)
    g["bucket"], g["dns_rcode"], g["drop_state"] = [0xFF, 0, 0xFF], 0xFF, 0xFFFF
    g["flows"][2] = 5
    h = nf.metrics_group_hash_content(2, g)
    assert h[0] == h[2] != h[1] and h[0] != 0 and nf.metrics_group_hash_content(3, g)[0] != h[0]
    assert (nf.metrics_group_hash_content(8, g) == 0).all()


def test_metrics_content_host_check_compiles_and_runs(nf, tmp_path):
    lib_dir = os.path.dirname(nf._lib.LIB_PATH)
    exe = str(tmp_path / "metrics_content_host_check")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "c", "metrics_content_host_check.c"), "-o", exe, "-L", lib_dir, "-lnfagg",
                           "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "metrics content host check ok", out.stderr


# ---- what must not have moved
def test_the_existing_abi_and_prom_counters_stay(nf):
    L = nf._lib
    assert L.DIM_ALL == (1 << 23) - 1 and L.lib.nfagg_abi_version() == 2 and nf.METRIC_GROUP.itemsize == 64
    want = {p + s for p in ("SrcK8S_", "DstK8S_") for s in nf.metrics.K8S_SUFFIXES} | {"SrcSubnetLabel", "DstSubnetLabel", "FlowDirection", "K8S_FlowLayer", "Proto"}
    assert set(nf.metrics.KEY_DIMS) == want and not set(nf.metrics.KEY_DIMS) & set(nf.metrics.CONTENT_KEY_DIMS)
    assert set(nf.metrics.CONTENT_KEY_DIMS) == {"DnsFlagsResponseCode", "PktDropLatestDropCause", "PktDropLatestState", "IPSecStatus"}
    g = nf.METRIC_GROUP_CONTENT
    assert g.itemsize == 128 and [g.fields[f][1] for f in g.names] == [0, 4, 8, 10, 12, 13, 14, 15, 16, 20, 22, 23, 24, 25, 32, 40, 48, 56, 64, 72, 88, 104]
    assert g.names[:8] == nf.METRIC_GROUP.names[:8] and [g.fields[f][1] for f in g.names[:8]] == [nf.METRIC_GROUP.fields[f][1] for f in g.names[:8]]
    for name in ("nfagg_metrics_table_create_specs", "nfagg_metrics_fold_content", "nfagg_metrics_fold_content_device", "nfagg_metrics_group_hash_content",
                 "nfagg_flp_enum_name"):
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    for item, message in ((dict(name="h", type="histogram", valueKey="Bytes"), "is not counter"), (dict(name="v", type="counter", valueKey="DnsLatencyMs"), "value key 'DnsLatencyMs'"),
                          (dict(name="k", type="counter", filters=[dict(key="DnsFlagsResponseCode", value="NoError", type="equal")]), "key 'DnsFlagsResponseCode' is outside")):
        with pytest.raises(ValueError) as e:
            nf.PromCounters([item])
        assert message in str(e.value)
    with nf.K8sTable([]) as k8s, nf.MetricsTable(k8s, [L.DIM_PROTO]) as plain:                # a plain table still builds as before
        assert plain.specs is None and plain.groupings == [L.DIM_PROTO]
