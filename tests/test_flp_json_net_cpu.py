"""direct-FLP JSON with direction, subnet labels and TCP flag names, CPU side: the restatement of tests/flp_json_net_ref.py
against the hand-derived vectors of tests/golden/net_vectors.json; nfagg_net_render against both; every error of
nfagg_net_table_create with no handle, each naming its entry; the ABI struct sizes and symbols; the longest lines of the
three policies, reached by the restatement; the CIDR helper; the exporters' argument rule."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_k8s_ref as K  # noqa: E402
import flp_json_net_ref as R  # noqa: E402
import k8s_cases as KC  # noqa: E402
import tls_worst_case as W  # noqa: E402
from flp_json_ref import marshal_sorted  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "net_vectors.json")))
ALL = dict(direction=True, flags=True)                       # with labels=...: every rule on
CAP_LABEL = b"\x01" * 42 + b"nnnn"                           # 42 x 6 + 4 = 256 escaped bytes: the cap


def latin(s):
    return None if s is None else s.encode("latin-1")


def flags_of(nf, rules):
    L = nf._lib
    return ((L.NET_REINTERPRET_DIRECTION if rules.get("direction") else 0) | (L.NET_SUBNET_LABELS if rules.get("labels") is not None else 0) |
            (L.NET_DECODE_TCP_FLAGS if rules.get("flags") else 0))


def net_table(nf, rules, table=None):
    """A NetTable of rules as the restatement takes them."""
    cats = [(R._b(name), texts) for name, texts in (rules.get("labels") or [])]
    return nf.NetTable(flags_of(nf, rules), cats, table)


def worst_case(nf, n, policy):
    """k8s_cases.worst_case (src == dst, host IP "h", not the reporter: FlowDirection 2; protocol 6 with flags 0xFFFF: all eleven
    names) plus a category whose name escapes to exactly the cap and holds the flow's address."""
    case = KC.worst_case(nf, n, policy)
    case["rules"] = dict(ALL, labels=[(CAP_LABEL, ["::/0"])])
    return case


def reference(case):
    """(bytes, offsets) of the restatement for a case of worst_case()."""
    present, parts, events = case["present"], case["parts"], None
    if case["answers"] is not None:
        present, drops, _rows, events, missing = W.RN.resolve(present, parts["network_events"], parts["drops"], case["answers"])
        assert not missing
        parts = {**parts, "drops": drops.view(parts["drops"].dtype).reshape(-1)}
    return R.encode(case["recs"], W.T.table_of(case["tls"]), K.table_of(case["k8s"]), case["layer"], case["rules"], case["now"], case["mono"],
                    case["names"], case["agent"], case["received"], present=present, parts=parts, events=events)


# ---- the restatement against the vectors
@pytest.mark.parametrize("case", GOLDEN["direction"], ids=[c["name"] for c in GOLDEN["direction"]])
def test_direction_truth_table_through_the_restatement(case):
    m = {b"AgentIP": latin(case["reporter"]), b"Flags": 16}
    for key, side in ((b"SrcK8S_HostIP", "src"), (b"DstK8S_HostIP", "dst")):
        if case[side] is not None:
            m[key] = latin(case[side])
    before = dict(m)
    out = R.reinterpret_direction(m)
    assert out.get(b"FlowDirection") == case["want"]
    assert {k: v for k, v in out.items() if k != b"FlowDirection"} == before and b"IfDirection" not in out
    if case["want"] is not None:                                   # a JSON integer, behind Flags in byte order
        assert b',"Flags":16,"FlowDirection":%d' % case["want"] in marshal_sorted(out)


def test_direction_rule_returns_at_an_empty_reporter():
    assert R.reinterpret_direction({b"AgentIP": b"", b"SrcK8S_HostIP": b"a", b"DstK8S_HostIP": b"a"}).get(b"FlowDirection") is None
    assert R.reinterpret_direction({b"SrcK8S_HostIP": b"a", b"DstK8S_HostIP": b"a"}).get(b"FlowDirection") is None


@pytest.mark.parametrize("case", GOLDEN["contains"], ids=["%s has %s" % (c["cidr"], c["ip"]) for c in GOLDEN["contains"]])
def test_containment_through_the_restatement(case):
    net_ip, mask = R.parse_cidr(case["cidr"])
    assert R.contains(net_ip, mask, R.parse_ip(case["ip"].encode())) is case["want"]


def test_first_match_and_the_empty_name_through_the_restatement():
    cats = R.parse_subnets([(latin(n), t) for n, t in GOLDEN["labels"]["categories"]])
    assert [n for n, _ in cats] == [latin(n) for n, t in GOLDEN["labels"]["categories"] if t]      # the one without CIDRs is dropped
    for case in GOLDEN["labels"]["cases"]:
        assert R.apply_subnet_label(case["ip"].encode(), cats) == latin(case["want"]), case
    rules = dict(R.RULES_OFF, labels=GOLDEN["labels"]["categories"])
    m = R.add_net({b"SrcAddr": b"10.1.2.3", b"DstAddr": b"192.168.1.7", b"SrcPort": 1, b"DstPort": 2, b"Etype": 2048}, rules, cats)
    assert marshal_sorted(m) == b'{"DstAddr":"192.168.1.7","DstPort":2,"Etype":2048,"SrcAddr":"10.1.2.3","SrcPort":1,"SrcSubnetLabel":"broad"}'
    assert R.add_net({b"Etype": 0x0806}, rules, cats) == {b"Etype": 0x0806}                        # not IP: no input key, no label


@pytest.mark.parametrize("case", GOLDEN["flags"], ids=[str(c["value"]) for c in GOLDEN["flags"]])
def test_flag_names_through_the_restatement(case):
    want = None if case["want"] is None else [latin(x) for x in case["want"]]
    assert R.decode_tcp_flags(case["value"]) == want
    line = marshal_sorted(R.add_net({b"Flags": case["value"], b"Etype": 1}, dict(R.RULES_OFF, flags=True), []))
    assert line == b'{"Etype":1,"Flags":' + (b"null" if want is None else b"[" + b",".join(b'"' + x + b'"' for x in want) + b"]") + b"}"
    assert R.add_net({b"Etype": 1}, dict(R.RULES_OFF, flags=True), []) == {b"Etype": 1}            # no Flags key: none appears


# ---- the host side of the library
def test_render_against_the_vectors_and_the_restatement(nf):
    cases = GOLDEN["labels"]["render"]
    cidrs = [(bytes(16), 0, 128, k) for k in range(len(cases))]
    with nf.NetTable(nf._lib.NET_SUBNET_LABELS, (cidrs, [latin(c["label"]) for c in cases]), raw=True) as t:
        for k, c in enumerate(cases):
            for side, want in ((0, latin(c["src"])), (1, latin(c["dst"]))):
                assert nf.net_render(t, side, k) == want == R.render(latin(c["label"]), side)
        want = R.render(latin(cases[0]["label"]), 0)
        L = nf._lib
        buf, n = np.full(len(want) + 8, 0xAB, dtype=np.uint8), C.c_size_t(0)
        call = lambda side, label, cap: L.lib.nfagg_net_render(t._t, side, label, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n))  # noqa: E731
        assert call(0, 0, len(want) - 1) == L.TRUNCATED and n.value == len(want) and (buf == 0xAB).all()
        assert L.lib.nfagg_net_render(t._t, 0, 0, None, 0, C.byref(n)) == L.TRUNCATED and n.value == len(want)
        assert call(0, 0, len(want)) == L.OK and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAB).all()
        assert call(0, len(cases) - 1, 0) == L.OK and n.value == 0                                 # the empty label: nothing
        assert call(2, 0, 64) == L.EINVAL and b"unknown side 2" in L.lib.nfagg_last_error(None)
        assert call(0, len(cases), 64) == L.EINVAL and b"label 4 of 4" in L.lib.nfagg_last_error(None)
        assert L.lib.nfagg_net_render(None, 0, 0, None, 0, C.byref(n)) == L.EINVAL


def test_every_byte_value_escapes_as_jsoniter_does(nf):
    label = bytes(range(1, 200))                                   # in two halves: the first escapes to 245 bytes, under the cap
    for part in (label[:100], label[100:]):
        with nf.NetTable(0, ([], [part]), raw=True) as t:
            assert nf.net_render(t, 0, 0) == R.render(part, 0) and nf.net_render(t, 1, 0) == R.render(part, 1)


def test_label_cap_at_256_and_257(nf):
    assert len(R.render(CAP_LABEL, 0)) == 18 + 2 + R.LABEL_MAX
    for ok in (CAP_LABEL, b"n" * 256):
        with nf.NetTable(0, ([], [b"first", ok]), raw=True) as t:
            assert nf.net_render(t, 1, 1) == R.render(ok, 1)
    for over, message in ((CAP_LABEL + b"n", "net label 1: its escaped value has 257 bytes, the cap is 256"),
                          (b'"' * 128 + b"n", "net label 1: its escaped value has 257 bytes, the cap is 256"),
                          (b"n" * 257, "net label 1: its escaped value has more than 256 bytes")):
        with pytest.raises(nf.NfaggError) as e:
            nf.NetTable(0, ([], [b"first", over]), raw=True)
        assert e.value.code == nf._lib.EINVAL and message in str(e.value), str(e.value)


V4 = bytes(10) + b"\xff\xff" + bytes([10, 0, 0, 0])


@pytest.mark.parametrize("cidrs, labels, message", [
    ([(V4, 8, 32, 0), (V4, 33, 32, 0)], [b"a"], "CIDR 1: a prefix of 33 in 32 bits"),
    ([(V4, 8, 32, 0), (bytes(16), 129, 128, 0)], [b"a"], "CIDR 1: a prefix of 129 in 128 bits"),
    ([(V4, 8, 64, 0)], [b"a"], "CIDR 0: 64 bits, neither 32 nor 128"),
    ([(V4, 0, 0, 0)], [b"a"], "CIDR 0: 0 bits, neither 32 nor 128"),
    ([(V4, 8, 32, 0), (V4, 8, 32, 0), (V4, 8, 32, 2)], [b"a", b"b"], "CIDR 2: label 2 of 2"),
    ([(V4, 8, 32, 0)], [], "CIDR 0: label 0 of 0"),
    ([(bytes(16), 8, 32, 0)], [b"a"], "CIDR 0: 32 bits and an address that is not v4-mapped"),
    ([(V4, 8, 32, 0)] * 1025, [b"a"], "1025 CIDRs, more than 1024"),
    ([], [b"a"] * 1025, "1025 labels, more than 1024"),
])
def test_table_errors_name_the_entry(nf, cidrs, labels, message):
    with pytest.raises(nf.NfaggError) as e:
        nf.NetTable(0, (cidrs, labels), raw=True)
    assert e.value.code == nf._lib.EINVAL and message in str(e.value), str(e.value)


def test_raw_table_errors_and_host_only_tables(nf):
    L = nf._lib
    t = C.c_void_p()
    rules = L.NetRules(struct_size=C.sizeof(L.NetRules))
    assert L.lib.nfagg_net_table_create(None, None, C.byref(t)) == L.EINVAL
    assert L.lib.nfagg_net_table_create(None, C.byref(rules), None) == L.EINVAL
    rules.struct_size = 8
    assert L.lib.nfagg_net_table_create(None, C.byref(rules), C.byref(t)) == L.EINVAL and b"struct_size" in L.lib.nfagg_last_error(None)
    rules = L.NetRules(struct_size=C.sizeof(L.NetRules), flags=8)
    assert L.lib.nfagg_net_table_create(None, C.byref(rules), C.byref(t)) == L.EINVAL and b"unknown net rule flags 0x8" in L.lib.nfagg_last_error(None)
    rules = L.NetRules(struct_size=C.sizeof(L.NetRules), n_cidrs=1)
    assert L.lib.nfagg_net_table_create(None, C.byref(rules), C.byref(t)) == L.EINVAL and b"null list with a count" in L.lib.nfagg_last_error(None)
    lab = (L.NetLabel * 1)()
    lab[0].len = 3                                                  # no pointer behind it
    rules = L.NetRules(struct_size=C.sizeof(L.NetRules), labels=lab, n_labels=1)
    assert L.lib.nfagg_net_table_create(None, C.byref(rules), C.byref(t)) == L.EINVAL and not t.value
    assert b"net label 0: null string with a length" in L.lib.nfagg_last_error(None)
    # the caps themselves are taken: 1024 CIDRs, every flag, zero CIDRs, no rule at all
    full = ([(V4, 8, 32, k % 3) for k in range(1024)], [b"a", b"", b"c"])
    with nf.NetTable(7, full, raw=True) as a, nf.NetTable(7) as b, nf.NetTable() as c, nf.TlsNames() as tls, nf.K8sTable([]) as k8s:
        assert (a.n_cidrs, a.n_labels, b.n_cidrs, c.flags) == (1024, 3, 0, 0)
        o, keep = nf.flp_options(agent_ip=bytes(16))
        off, need = np.zeros(2, dtype=np.uint64), C.c_size_t(7)
        for fn in (L.lib.nfagg_encode_flp_json_net, L.lib.nfagg_encode_flp_json_net_device):
            # no handle: the call ends at its argument checks, before any device work
            for net in (a._t, None):
                assert fn(None, None, 0, None, None, None, tls._t, k8s._t, net, C.byref(o), None, 0, off.ctypes.data_as(C.c_void_p), C.byref(need)) == L.EINVAL
            assert fn(None, None, 0, None, None, None, tls._t, k8s._t, a._t, None, None, 0, off.ctypes.data_as(C.c_void_p), C.byref(need)) == L.EINVAL
            assert b"null options" in L.lib.nfagg_last_error(None)
        rows = np.zeros(2, dtype=np.uint64)
        for fn in (L.lib.nfagg_net_resolve, L.lib.nfagg_net_resolve_device):
            assert fn(None, a._t, k8s._t, None, 0, None, C.byref(o), rows.ctypes.data_as(C.c_void_p)) == L.EINVAL


def test_sizes_and_symbols(nf):
    L = nf._lib
    assert C.sizeof(L.FlpOptions) == 80 and L.lib.nfagg_abi_version() == 2
    assert (C.sizeof(L.NetCidr), C.sizeof(L.NetLabel), C.sizeof(L.NetRules), C.sizeof(L.NetRow)) == (28, 16, 32, 8)
    assert (L.NetCidr.ones.offset, L.NetCidr.label.offset, L.NetRules.cidrs.offset, L.NetRules.n_labels.offset, L.NetRow.direction.offset) == (16, 24, 8, 28, 4)
    assert nf.NET_ROW.itemsize == 8 and nf.NET_ROW.fields["direction"][1] == 4
    assert (L.NET_REINTERPRET_DIRECTION, L.NET_SUBNET_LABELS, L.NET_DECODE_TCP_FLAGS) == (1, 2, 4)
    assert (L.NET_MAX_CIDRS, L.NET_LABEL_MAX, L.NET_NO_LABEL, L.NET_NO_DIRECTION) == (R.MAX_CIDRS, R.LABEL_MAX, R.NO_LABEL, R.NO_DIRECTION) == (1024, 256, 0xFFFF, 0xFF)
    for sym in ("nfagg_net_table_create", "nfagg_net_table_destroy", "nfagg_net_render", "nfagg_net_resolve", "nfagg_net_resolve_device",
                "nfagg_encode_flp_json_net", "nfagg_encode_flp_json_net_device", "nfagg_flp_json_net_max_line"):
        assert getattr(L.lib, sym) is not None and sym in L.SIGNATURES
    header = open(os.path.join(os.path.dirname(HERE), "include", "nfagg.h")).read()
    for text in ("NFAGG_NET_MAX_CIDRS 1024", "NFAGG_NET_LABEL_MAX 256", "NFAGG_NET_REINTERPRET_DIRECTION 1u", "NFAGG_NET_SUBNET_LABELS 2u",
                 "NFAGG_NET_DECODE_TCP_FLAGS 4u", "transform_network_direction.go:32-64", "transform_network.go:129-146", "utils/tcp_flags.go:8-48",
                 "reflect_slice.go:28-29"):
        assert text in header, text


@pytest.mark.parametrize("policy", [0, 1, 2])
def test_longest_line_is_reached_by_the_restatement(nf, policy):
    """The write kernels size their LDS windows by nfagg_flp_json_net_max_line: the longest enriched line, two label fragments at
    the cap, the direction key and the eleven flag names in place of five digits. The restatement's line for the worst-case flow
    has exactly that many bytes, the table takes that flow's rules, and the window keeps its 16 KiB."""
    case = worst_case(nf, 1, policy)
    buf, off = reference(case)
    net_table(nf, case["rules"]).close()
    lib = nf._lib.lib
    names = b'["FIN","SYN","RST","PSH","ACK","URG","ECE","CWR","SYN_ACK","FIN_ACK","RST_ACK"]'
    grow = 2 * (len(b',"SrcSubnetLabel":""') + 256) + len(b',"FlowDirection":2') + len(names) - 5
    assert len(buf) == lib.nfagg_flp_json_net_max_line(policy) == lib.nfagg_flp_json_k8s_max_line(policy) + grow and grow == 644
    assert lib.nfagg_flp_json_net_max_line(3) == 0 and lib.nfagg_flp_json_net_max_line(-1) == 0
    assert b',"Flags":' + names + b',"FlowDirection":2,' in buf and buf.count(b'SubnetLabel":"\\u0001') == 2
    window = (32768 - (16 if policy == 0 else 2048) - (len(buf) + 15) // 16 * 16) // 16 * 16
    assert window >= 16384


def test_cidr_helper(nf):
    cidrs, labels = nf.net_cidrs([("a", ["10.1.2.3/8", "::ffff:10.0.0.0/104"]), ("none", []), (b"b\xff", ["2001:db8::/32"])])
    assert labels == [b"a", b"b\xff"]
    assert cidrs == [(V4[:13] + bytes([1, 2, 3]), 8, 32, 0), (V4, 104, 128, 0), (bytes.fromhex("20010db8") + bytes(12), 32, 128, 1)]
    for bad in ("10.0.0.0", "10.0.0.0/33", "::/129", "10.0.0.0/x", "nonsense/8"):
        with pytest.raises(ValueError):
            nf.net_cidrs([("a", [bad])])


def test_exporters_want_k8s_with_net(nf):
    calls = []

    class Table:
        encode_flp_json = None

        def encode_flp_json_net(self, raw, tls_names, k8s, net, now_ns, mono_ns, names, agent_ip, time_received, unknown):
            calls.append((len(raw), tls_names, k8s, net, now_ns, mono_ns, time_received))
            return np.frombuffer(b"a\nb\n", dtype=np.uint8), np.array([0, 2, 4], dtype=np.uint64)

    import io
    out = io.BytesIO()
    with pytest.raises(ValueError):
        nf.StartDirectFLPJSON(Table(), out, agent_ip=bytes(16), tls_names="names", net="rules")
    exp = nf.StartDirectFLPJSON(Table(), out, agent_ip=bytes(16), time_received=lambda: 5, tls_names="names", k8s="table", net="rules")
    assert exp.ExportEvicted(np.zeros(2, dtype=nf.FLOW_RECORD), 11, 13) == 2
    assert calls == [(2, "names", "table", "rules", 11, 13, 5)] and out.getvalue() == b"a\nb\n" and (exp.lines, exp.deferred) == (2, 0)
    mt = nf.MapTracer(nf.GPUMapFetcher(None, lambda: None), 0, 0)
    with pytest.raises(ValueError):
        mt.evictFlowsJSON(tls_names="names", net="rules")
