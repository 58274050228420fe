"""`extract timebased` without a GPU: the restatement of tests/timebased_ref.py against the hand-worked vectors of
tests/golden/timebased_vectors.json; parse_rules on good and skipped rules; what nfagg_timebased_rules_create(h = NULL) checks;
the signatures; the rendering of key read-backs from hand-made nfagg_tb_key values."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timebased_ref as T  # noqa: E402

S = 10**9
VECTORS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "timebased_vectors.json")))["vectors"]


def canon(maps):
    return sorted(json.dumps(m, sort_keys=True) for m in maps)


# ---- 1. the restatement against the hand-worked vectors
@pytest.mark.parametrize("vec", VECTORS, ids=[v["name"] for v in VECTORS])
def test_restatement_against_hand_worked_vectors(vec):
    ref = T.Timebased(vec["rules"])
    for call in vec["calls"]:
        got = ref.extract(call["flows"], call["now"])
        assert len(ref.per_rule) == len(call["expect"]) == len(vec["rules"])
        for ru, mine, want in zip(vec["rules"], ref.per_rule, call["expect"]):
            if ru.get("topK"):
                assert mine == want, (vec["name"], call["now"], ru["name"])
            else:
                assert canon(mine) == canon(want), (vec["name"], call["now"], ru["name"])
            for a, b in zip(sorted(mine, key=lambda m: json.dumps(m, sort_keys=True)), sorted(want, key=lambda m: json.dumps(m, sort_keys=True))):
                assert T.same_bits(a[ru["operationKey"]], b[ru["operationKey"]])
        assert got == [m for maps in ref.per_rule for m in maps]


def test_the_restatement_panics_on_a_missing_operation_key():
    ref = T.Timebased([dict(name="r", indexKeys=["SrcAddr"], operationType="sum", operationKey="Bytes", timeInterval=S)])
    with pytest.raises(T.MissingKeyPanic):
        ref.extract([{"SrcAddr": "A"}], 0)
    ref = T.Timebased([dict(name="r", indexKeys=["SrcAddr"], operationType="count", operationKey="Bytes", timeInterval=S)])
    with pytest.raises(T.MissingKeyPanic):                                # count converts the value too (filters.go:86-91)
        ref.extract([{"SrcAddr": "A"}], 0)
    assert T.Timebased([dict(name="r", indexKeys=["DstAddr"], operationType="sum", operationKey="Bytes")]).extract([{"SrcAddr": "A"}], 0) == []


def test_the_heap_keeps_the_k_best_whatever_the_order():
    rng = np.random.default_rng(5)
    for bottom in (False, True):
        for k in (1, 3, 10, 40):
            vals = rng.integers(-5, 6, 30).astype(float)
            res = {"k%d" % i: v for i, v in enumerate(vals)}
            got = T.top_or_bottom_k(res, k, bottom)
            assert [v for _, v in got] == sorted(vals, reverse=not bottom)[:k]
            assert len({key for key, _ in got}) == len(got) and all(res[key] == v for key, v in got)


# ---- 2. parse_rules
def test_parse_rules_good_and_skipped(nf):
    cfg = dict(rules=[
        dict(name="a", indexKeys=["SrcAddr", "DstAddr"], operationType="sum", operationKey="Bytes", topK=10, timeInterval="1m"),
        dict(name="b", indexKey="SrcAddr", operationType="last", operationKey="Packets", reversed=True, timeInterval="1500ms"),
        dict(name="none", operationType="sum", operationKey="Bytes"),
        dict(name="bad", indexKey="SrcAddr", operationType="median", operationKey="Bytes", timeInterval="1h"),
        dict(name="c", indexKeys=["SrcAddr"], indexKey="ignored", operationType="count", operationKey="Bytes", timeInterval=5),
    ])
    rules, skipped, tables = nf.parse_rules(cfg)
    assert [r["name"] for r in rules] == ["a", "b", "c"]
    assert rules[0] == dict(name="a", index_key="SrcAddr,DstAddr", index_keys=["SrcAddr", "DstAddr"], operation="sum", operation_key="Bytes", top_k=10,
                            reversed=False, interval_ns=60 * S)
    assert rules[1]["index_keys"] == ["SrcAddr"] and rules[1]["reversed"] and rules[1]["interval_ns"] == 1_500_000_000 and rules[1]["top_k"] == 0
    assert rules[2]["index_key"] == "SrcAddr" and rules[2]["interval_ns"] == 5
    assert [(it["name"], why) for it, why in skipped] == [("none", "missing IndexKey(s)"), ("bad", "illegal operation type median")]
    # the rule dropped for its operation has created its table and widened it by then (timebased.go:66-79)
    assert tables == {"SrcAddr,DstAddr": 60 * S, "SrcAddr": 3600 * S}
    assert nf.parse_rules(cfg["rules"])[0] == rules
    ref = T.Timebased([dict(r, timeInterval=nf.conntrack.parse_duration(r.get("timeInterval") or 0)) for r in cfg["rules"]])
    assert [f["rule"]["name"] for f in ref.filters] == ["a", "b", "c"] and {k: t["max_interval"] for k, t in ref.tables.items()} == tables


# ---- 3. nfagg_timebased_rules_create(h = NULL)
ENTRIES = [("10.0.0.1", dict(namespace="shop", name="a", kind="Pod")), ("10.0.0.2", dict(namespace="a,b", name="b", kind="Pod", host_ip="1.2.3.4", host_name="n,1")),
           ("10.0.0.3", dict(name="c", kind="Node"))]


def create(nf, rules, k8s=None, net=None, max_keys=16, options=None):
    return nf.TimebasedRules(rules, k8s, net, max_keys, None, options)


def refused(nf, needle, rules, **kw):
    with pytest.raises(nf.NfaggError) as e:
        create(nf, rules, **kw)
    assert e.value.code == nf._lib.EINVAL and needle in str(e.value), str(e.value)


def test_rules_create_on_the_host_alone(nf):
    L = nf._lib
    with nf.K8sTable(ENTRIES[:1] + ENTRIES[2:], None, None) as k8s, nf.NetTable(L.NET_SUBNET_LABELS, [(b"east", ["10.0.0.0/8"]), (b"", ["11.0.0.0/8"])], None) as net:
        every = ["SrcAddr", "DstAddr", "SrcPort", "DstPort", "Proto", "SrcSubnetLabel", "DstSubnetLabel", "FlowDirection"] + \
                ["%sK8S_%s" % (s, f) for s in ("Src", "Dst") for f in nf.metrics.K8S_SUFFIXES]
        for key in every:
            with create(nf, [dict(index_keys=[key], interval_ns=S)], k8s, net) as tb:
                st = tb.stats()
                assert (st.n_tables, st.n_rules, st.failed, st.has_clock) == (1, 1, 0, 0) and tb.table_of_rule == [0]
        # rules with equal key lists share a table; the widest key; sixteen rules
        rules = [dict(index_keys=["SrcAddr", "DstAddr", "SrcPort", "DstPort"], operation=op, value=L.MET_VALUE_BYTES, top_k=L.TB_MAX_TOPK) for op in range(1, 8)] + \
                [dict(index_keys=["SrcAddr"], value=v) for v in (1, 2, 3, 4)] + [dict(index_keys=["Proto"]), dict(index_keys=["SrcK8S_Namespace", "DstK8S_Namespace"])] * 2 + \
                [dict(index_keys=["Proto"], reversed=True)]
        with create(nf, rules, k8s, net, max_keys=L.TB_MAX_KEYS) as tb:
            assert tb.table_of_rule == [0] * 7 + [1] * 4 + [2, 3, 2, 3, 2] and tb.stats().n_tables == 4
            assert tb.key_hash(0, np.zeros(2, dtype=nf.TB_KEY))[0] == tb.key_hash(0, np.zeros(1, dtype=nf.TB_KEY))[0] != 0
            with pytest.raises(nf.NfaggError) as e:                       # a host-only object holds no key
                tb.keys(0, [0])
            assert "host alone" in str(e.value)


def test_rules_create_refuses(nf):
    L = nf._lib
    ok = dict(index_keys=["SrcAddr"], interval_ns=S)
    with nf.K8sTable(ENTRIES, None, None) as k8s, nf.K8sTable(ENTRIES[:1], None, None) as k8s_plain, \
            nf.NetTable(L.NET_SUBNET_LABELS, [(b"east,west", ["10.0.0.0/8"])], None) as net, nf.NetTable(L.NET_SUBNET_LABELS, [(b"east", ["10.0.0.0/8"])], None) as net_plain:
        # every refused key name, by its name
        for key in ("Bytes", "srcaddr", "SrcAddr ", "", "SrcK8S_", "SrcK8S_Labels", "K8S_FlowLayer", "SrcMac", "Interfaces", "IcmpType", "DnsId", "_HashId", "SrcK8S_Namespace,DstK8S_Namespace"):
            refused(nf, 'rule 1: index key "%s" is not served' % key, [ok, dict(index_keys=[key])], k8s=k8s_plain, net=net_plain)
        refused(nf, 'rule 0: index key "DstK8S_Zone" needs the Kubernetes table', [dict(index_keys=["DstK8S_Zone"])])
        refused(nf, 'rule 0: index key "DstSubnetLabel" needs the net table', [dict(index_keys=["DstSubnetLabel"])], k8s=k8s_plain)
        create(nf, [dict(index_keys=["FlowDirection"])]).close()         # the direction needs no table
        # a ',' in a selected text
        refused(nf, 'index key "SrcK8S_Namespace": the text "a,b" contains \',\'', [dict(index_keys=["SrcK8S_Namespace"])], k8s=k8s)
        refused(nf, 'index key "DstK8S_HostName": the text "n,1" contains \',\'', [ok, dict(index_keys=["Proto", "DstK8S_HostName"])], k8s=k8s)
        create(nf, [dict(index_keys=["SrcK8S_Name"])], k8s=k8s).close()  # another field of the same rows is fine
        refused(nf, "the text of label 0 contains ','", [dict(index_keys=["SrcSubnetLabel"])], net=net)
        create(nf, [dict(index_keys=["FlowDirection"])], net=net).close()
        # each cap exceeded by one
        refused(nf, "17 rules, not 1..16", [ok] * 17)
        refused(nf, "0 rules, not 1..16", [])
        refused(nf, "rule 4: more than 4 distinct index-key lists", [dict(index_keys=[k]) for k in ("SrcAddr", "DstAddr", "Proto", "SrcPort", "DstPort")])
        refused(nf, 'rule 4: table "SrcAddr" has more than 4 value sources', [dict(index_keys=["SrcAddr"], value=v) for v in (1, 2, 3, 4, 5)])
        refused(nf, "rule 0: 5 index keys, not 1..4", [dict(index_keys=["Proto"] * 4, n_index_keys=5)])
        refused(nf, "rule 0: 0 index keys, not 1..4", [dict(index_keys=[])])
        refused(nf, "rule 0: the index keys take 48 bytes, more than 40", [dict(index_keys=["SrcAddr", "DstAddr", "SrcAddr"])])
        refused(nf, "rule 0: top_k 4097, more than 4096", [dict(ok, top_k=L.TB_MAX_TOPK + 1)])
        refused(nf, "max_keys 16777217, not 1..16777216", [ok], max_keys=L.TB_MAX_KEYS + 1)
        refused(nf, "max_keys 0, not 1..16777216", [ok], max_keys=0)
        refused(nf, "rule 1: unknown operation 8", [ok, dict(ok, operation=8)])
        refused(nf, "rule 0: unknown operation 0", [dict(ok, operation=0)])
        refused(nf, "rule 0: unknown value source 7", [dict(ok, value=7)])
        refused(nf, "rule 0: unknown value source 0", [dict(ok, value=0)])
        refused(nf, "rule 0: a negative interval", [dict(ok, interval_ns=-1)])
        # a wrong struct_size
        refused(nf, "rule 1: struct_size 47, not 64", [ok, dict(ok, struct_size=C.sizeof(L.TbRule) - 17)])
        refused(nf, "nfagg_tb_options.struct_size 4, not 8", [ok], options=L.TbOptions(4, 16))
    assert C.sizeof(L.TbRule) == 64 and C.sizeof(L.TbOptions) == 8 and nf.TB_RESULT.itemsize == 16 and nf.TB_KEY.itemsize == 64


def test_a_host_only_object_serves_no_call(nf):
    with create(nf, [dict(index_keys=["SrcAddr"])]) as tb:
        tb.reset()
        caps, n_out, outs, missing = (C.c_uint32 * 1)(4), (C.c_uint32 * 1)(), (C.c_void_p * 1)(), C.c_uint64(0)
        for rc in (nf._lib.lib.nfagg_timebased_extract(None, tb._t, None, 0, None, None, None, 0, caps, outs, n_out, C.byref(missing)),
                   nf._lib.lib.nfagg_timebased_results(None, tb._t, caps, outs, n_out)):
            assert rc == nf._lib.EINVAL


# ---- 4. the signatures
def test_signatures(nf):
    sig = nf._lib.SIGNATURES
    names = ["nfagg_timebased_rules_create", "nfagg_timebased_destroy", "nfagg_timebased_extract", "nfagg_timebased_extract_device", "nfagg_timebased_results",
             "nfagg_timebased_results_device", "nfagg_timebased_keys", "nfagg_timebased_class_row", "nfagg_timebased_key_hash", "nfagg_timebased_reset",
             "nfagg_timebased_stats"]
    for n in names:
        assert n in sig and hasattr(nf._lib.lib, n), n
    assert len(sig["nfagg_timebased_extract"][1]) == len(sig["nfagg_timebased_extract_device"][1]) == 12
    assert len(sig["nfagg_timebased_results"][1]) == 5 and sig["nfagg_timebased_destroy"][0] is None
    assert (nf.EDEFER, nf._lib.TB_INEXACT) == (3, 1)
    assert C.sizeof(nf._lib.TbStats) == 8 + 3 * 16 + 64 + 8 + 8 + 8
    assert callable(nf.FlowTable.timebased_rules) and callable(nf.FlowTable.timebased_extract)
    assert issubclass(nf.MissingOperationKey, RuntimeError) and issubclass(nf.TimebasedOverflow, RuntimeError)


# ---- 5. rendering of key read-backs
class _FakeRules:
    """What render_column reads of a TimebasedRules."""

    def __init__(self, k8s, net, rows):
        self.k8s, self.net, self.rows = k8s, net, rows

    def class_row(self, table, column, cls):
        return self.rows[(table, column, cls)]


def tb_key(*cols):
    k = np.zeros(1, dtype=np.dtype([("col", "u1", (4, 16))]))
    for c, v in enumerate(cols):
        raw = v if isinstance(v, bytes) else struct.pack("<I", v) + bytes(12)
        k["col"][0, c] = np.frombuffer(raw, dtype=np.uint8)
    return k[0]


def test_rendering_of_key_read_backs(nf):
    from netobserv_ebpf_agent_amd.timebased import render_column
    L = nf._lib
    v4 = bytes(10) + b"\xff\xff" + bytes([10, 1, 2, 3])
    v6 = bytes.fromhex("20010db8000000000000000000000001")
    with nf.K8sTable(ENTRIES, None, None) as k8s, nf.NetTable(L.NET_SUBNET_LABELS, [(b"east", ["10.0.0.0/8"]), (b"w\xc3\xa9st", ["11.0.0.0/8"])], None) as net:
        fake = _FakeRules(k8s, net, {(0, 2, 1): 0, (0, 2, 2): 1, (0, 3, 1): 1})
        key = tb_key(v4, v6, 2, 1)
        assert render_column("SrcAddr", key["col"][0], fake, 0, 0) == "10.1.2.3"
        assert render_column("DstAddr", key["col"][1], fake, 0, 1) == "2001:db8::1"
        assert render_column("DstAddr", bytes(16), fake, 0, 1) == "::"
        assert render_column("SrcK8S_Namespace", key["col"][2], fake, 0, 2) == "a,b" and render_column("SrcK8S_Name", tb_key(0, 0, 1)["col"][2], fake, 0, 2) == "a"
        assert render_column("DstK8S_HostName", key["col"][3], fake, 0, 3) == "n,1"
        key = tb_key(65535, 0, 132, 1)
        assert [render_column(k, key["col"][c], fake, 0, c) for c, k in enumerate(("SrcPort", "DstPort", "Proto", "FlowDirection"))] == ["65535", "0", "132", "1"]
        assert render_column("SrcSubnetLabel", tb_key(1)["col"][0], fake, 0, 0) == "wést" and render_column("DstSubnetLabel", tb_key(0)["col"][0], fake, 0, 0) == "east"
