"""transform filter, CPU side: the query language's lexer and parser against hand-worked vectors (precedence, keyword case, raw
strings, escapes, every error class with its line:column); the compiler's atoms, ops and steps for the shapes the reference
answers in surprising ways, and every refused shape; the restatement of tests/flp_filter_ref.py on hand-built maps; the roll,
equal between the library, the product's Python and the restatement, and binomial within five sigma; host-only filters over
host-only tables; tools/c/filter_host_check.c compiled and run against the library (no handle)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_filter_ref as FR  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def cmp(key, op, value):
    return ("cmp", key, op, value)


A, B, C3 = cmp("a", "=", 1), cmp("b", "=", 2), cmp("c", "=", 3)


# ---- lexer and parser
@pytest.mark.parametrize("text, tree", [
    ("a = 1 and b = 2 or c = 3", ("and", A, ("or", B, C3))),                    # expr.y:16-17: OR binds tighter than AND
    ("a = 1 or b = 2 and c = 3", ("and", ("or", A, B), C3)),
    ("a = 1 and b = 2 and c = 3", ("and", ("and", A, B), C3)),                  # left-associative, both
    ("a = 1 or b = 2 or c = 3", ("or", ("or", A, B), C3)),
    ("(a = 1 and b = 2) or c = 3", ("or", ("and", A, B), C3)),
    ("a = 1 or (b = 2 and (c = 3))", ("or", A, ("and", B, C3))),
    ("((a = 1))", A),
    ("a = 1 AND b = 2 Or c = 3", ("and", A, ("or", B, C3))),                    # lexer.go:211: any letter case
    ("WITH(a) and wiThouT(b)", ("and", ("with", "a"), ("without", "b"))),
    ('k = "x y"', cmp("k", "=", b"x y")),
    ('k != "a\\tb\\"c\\\\\\x41\\101\\u00e9"', cmp("k", "!=", b'a\tb"c\\AA\xc3\xa9')),
    ("k =~ `a\\.b`", cmp("k", "=~", b"a\\.b")),                                # a raw string: no escapes
    ('k !~ "^x$"', cmp("k", "!~", b"^x$")),
    ("k>=10 and k<=20 and k<5 and k>7 and k!=3", ("and", ("and", ("and", ("and", cmp("k", ">=", 10), cmp("k", "<=", 20)), cmp("k", "<", 5)), cmp("k", ">", 7)),
                                                  cmp("k", "!=", 3))),
    ("a = 1 // trailing\n and /* inner */ b = 2", ("and", A, B)),               # comments are skipped
    ("a = 017", cmp("a", "=", 17)),                                             # ParseInt(s, 10, 64) of an octal-looking literal
    ("a = 9223372036854775807", cmp("a", "=", 2**63 - 1)),
    ("SrcK8S_Namespace = \"\"", cmp("SrcK8S_Namespace", "=", b"")),
])
def test_parse_vectors(nf, text, tree):
    assert nf.parse_query(text) == tree


@pytest.mark.parametrize("text, message", [
    ("a = 1.5", "Float values are currently unsupported: 1:5"),
    ("a = 1e3", "Float values are currently unsupported: 1:5"),
    ("a > -1", "syntax error: unexpected NF_FIELD: 1:5"),                      # no unary minus: '-' is a field name
    ('a = "abc', "invalid syntax: 1:5"),                                       # strconv.Unquote of a literal that is not terminated
    ("a = `abc", "invalid syntax: 1:5"),
    ("a = 0x10", 'strconv.ParseInt: parsing "0x10": invalid syntax: 1:5'),
    ("a = 9223372036854775808", "value out of range: 1:5"),
    ("a = 1 b = 2", "syntax error: unexpected NF_FIELD: 1:7"),
    ("a =", "syntax error: unexpected $end: 1:3"),
    ("a = 1 and", "syntax error: unexpected $end: 1:9"),
    ("a < \"x\"", "syntax error: unexpected STRING: 1:5"),
    ("a =~ 5", "syntax error: unexpected NUMBER: 1:6"),
    ("with a", "syntax error: unexpected NF_FIELD: 1:6"),
    ("with(\"a\")", "syntax error: unexpected STRING: 1:6"),
    ("(a = 1", "syntax error: unexpected $end: 1:6"),
    ("a = 1)", "syntax error: unexpected CLOSE_PARENTHESIS: 1:6"),
    ("a == 1", "syntax error: unexpected EQ: 1:4"),
    ("a = 1\nand b = 2.0", "Float values are currently unsupported: 2:9"),
    ("", "syntax error: unexpected $end: 0:0"),                                # scanner.go: no character read yet, so line - 1 and column 0
    ('a =~ "("', "invalid regex filter"),
    ('a = "\\q"', "invalid syntax: 1:5"),
])
def test_parse_errors(nf, text, message):
    with pytest.raises(ValueError) as e:
        nf.parse_query(text)
    assert message in str(e.value)


# ---- the restatement on hand-built maps
def test_restatement_on_hand_built_maps(nf):
    P = nf.parse_query
    m = {b"Bytes": 2**63, b"Proto": 6, b"Flags": [b"SYN"], b"SrcK8S_Name": b"pod", b"Port": b"443", b"SrcAddr": b"10.0.0.1", b"Interfaces": [b"eth0", b"lo"]}
    ev = lambda q: FR.evaluate(P(q), m)  # noqa: E731
    assert ev("Bytes < 0") and not ev("Bytes > 0")                               # uint64 wraps into int
    assert not ev('Proto = "6"') and ev('Proto != "6"') and ev("Proto = 6") and ev('Proto =~ "^6$"')
    assert not ev("Flags > 0") and not ev("Flags < 1") and not ev('Flags = "SYN"') and ev("with(Flags)") and ev('Flags =~ "^.SYN.$"')
    assert ev('Missing != "x"') and not ev("Missing != 1") and not ev('Missing !~ "x"') is False
    assert ev("Port >= 443") and ev('SrcK8S_Name =~ "o"') and not ev('SrcK8S_Name =~ "^o"')
    assert ev('Interfaces =~ "^.eth0 lo.$"') and not ev("Interfaces = 1")
    assert ev("Proto = 17 and Proto = 6 or Proto = 6") is False                  # a and (b or c)
    cfg = dict(rules=[dict(type="remove_entry_if_equal", removeEntry=dict(input="Proto", value=6))])
    assert FR.transform(cfg, m, P, 0, 0)[0] == 1                                  # a YAML number never equals a uint8
    cfg = dict(rules=[dict(type="remove_entry_if_not_equal", removeEntry=dict(input="Proto", value=6))])
    assert FR.transform(cfg, m, P, 0, 0)[0] == 0
    cfg = dict(rules=[dict(type="remove_entry_if_equal", removeEntry=dict(input="SrcK8S_Name", value="pod"))])
    assert FR.transform(cfg, m, P, 0, 0)[0] == 0
    cfg = dict(rules=[dict(type="remove_entry_all_satisfied", removeEntryAllSatisfied=[])])
    assert FR.transform(cfg, m, P, 0, 0)[0] == 0
    two = dict(samplingField="Sampling", rules=[dict(type="keep_entry_query", keepEntryQuery="Proto = 6", keepEntrySampling=3),
                                                dict(type="remove_entry_if_doesnt_exist", removeEntry=dict(input="Sampling")),
                                                dict(type="keep_entry_query", keepEntryQuery="with(Bytes)")])
    seen = set()
    for i in range(64):
        k, r, out = FR.transform(two, m, P, 5, i)
        seen.add((k, r, out.get(b"Sampling") if out else None))
    assert seen == {(1, 0, 3), (0, 1, None)}              # admitted by rule 0: stored; sampled out, admitted by rule 1: no Sampling, removed


# ---- the compiler
def compiled(nf, rules, **kw):
    return nf.TransformFilter(dict(rules=rules, samplingField=kw.pop("samplingField", "")), **kw)


def keep(q, sampling=0):
    return dict(type="keep_entry_query", keepEntryQuery=q, keepEntrySampling=sampling)


ENTRIES = [("10.0.0.1", dict(namespace="ns1", name="a", kind="Pod", host_ip="192.168.0.1", host_name="n1", zone="z")),
           ("10.0.0.2", dict(namespace="", name="42", kind="Node")),
           ("10.0.0.3", dict(namespace="ns2", name="-7", kind="Pod", zone=""))]
LABELS = [b"inside", b"", b"17"]


def test_compile_vectors(nf):
    F = nf.filter
    t = compiled(nf, [keep('Proto = "6"')])
    assert t.atoms == [dict(kind=F.ATOM_CONST, value_const=0)] and bytes(t.ops) == b"\x00" and t.steps == [(F.STEP_KEEP, 0, 0, 0, 1)]
    t = compiled(nf, [keep('Proto != "6"')])                                        # true for an absent key too
    assert t.atoms == [dict(kind=F.ATOM_CONST, value_const=0)] and bytes(t.ops) == bytes([0, F.OP_NOT])
    t = compiled(nf, [keep("DnsId != 5")])                                          # NumNotEquals: false for an absent key, no negation
    assert t.atoms == [dict(kind=F.ATOM_NUM, field=16, cmp=1, value=5)] and bytes(t.ops) == bytes([0])
    t = compiled(nf, [dict(type="remove_entry_if_equal", removeEntry=dict(input="Proto", value=6))])
    assert t.atoms == [dict(kind=F.ATOM_CONST, value_const=0)] and t.steps == [(F.STEP_REMOVE, 0, 0, 0, 1)]
    t = compiled(nf, [dict(type="remove_entry_if_not_equal", removeEntry=dict(input="Proto", value=6.0))])
    assert t.atoms == [dict(kind=F.ATOM_PRESENT, field=4)]
    t = compiled(nf, [keep("with(Interfaces) and without(SrcMac) or with(TimeReceived)")])
    assert t.atoms == [dict(kind=F.ATOM_CONST, value_const=1)] and bytes(t.ops) == bytes([0, 0, F.OP_NOT, 0, F.OP_OR, F.OP_AND])
    t = compiled(nf, [keep('SrcAddr = "10.0.0.1" or SrcAddr = "010.0.0.1" or DstAddr = "::ffff:10.0.0.1" or DstAddr = "2001:DB8::1" or DstAddr = "2001:db8:0:0:1::1"')])
    assert [a["kind"] for a in t.atoms] == [F.ATOM_ADDR, F.ATOM_CONST] and t.atoms[0]["bytes"] == bytes(10) + b"\xff\xff\x0a\x00\x00\x01" and t.atoms[0]["side"] == 0
    t = compiled(nf, [keep('DstAddr = "2001:db8::1:0:0:1" and SrcMac = "0a:1b:2c:3d:4e:5f" and DstMac = "0A:1B:2C:3D:4E:5F" and SrcAddr > 5')])
    assert [a["kind"] for a in t.atoms] == [F.ATOM_ADDR, F.ATOM_MAC, F.ATOM_CONST] and t.atoms[1]["bytes"] == bytes.fromhex("0a1b2c3d4e5f") and t.atoms[0]["side"] == 1
    t = compiled(nf, [keep("Flags > 0 and with(Flags)")], net_flags=nf._lib.NET_DECODE_TCP_FLAGS)      # the kernel answers: the spec is the same
    assert t.atoms == [dict(kind=F.ATOM_NUM, field=10, cmp=3, value=0), dict(kind=F.ATOM_PRESENT, field=10)]
    # table-backed keys: one truth byte per row and one for "no row"
    t = compiled(nf, [keep('SrcK8S_Namespace = "ns1" and DstK8S_Name >= 0 and SrcK8S_Zone =~ "^$" and without(DstK8S_HostName) and DstSubnetLabel != "inside"'
                           ' and SrcSubnetLabel > 16 and K8S_FlowLayer = "app" and DnsFlagsResponseCode =~ "^Form" and IPSecStatus = "error"')],
                 k8s_entries=ENTRIES, labels=LABELS, layer=True)
    truths = [(a["dim"], a["truth"]) for a in t.atoms]
    assert truths[0] == (F.DIM_SRC_K8S_ROW, bytes([1, 0, 0, 0])) and truths[1] == (F.DIM_DST_K8S_ROW, bytes([0, 1, 0, 0]))
    assert truths[2] == (F.DIM_SRC_K8S_ROW, bytes([0, 0, 1, 0])) and truths[3] == (F.DIM_DST_K8S_ROW, bytes([1, 0, 0, 0]))
    assert truths[4] == (F.DIM_DST_SUBNET_LABEL, bytes([1, 0, 0, 0])) and truths[5] == (F.DIM_SRC_SUBNET_LABEL, bytes([0, 0, 1, 0]))
    assert truths[6] == (F.DIM_FLOW_LAYER, bytes([0, 1, 0])) and truths[8] == (F.DIM_IPSEC_STATUS, bytes([0, 1, 0]))
    assert truths[7][0] == F.DIM_DNS_RCODE and len(truths[7][1]) == 17 and truths[7][1][0] == 0 and truths[7][1][1] == 1 and truths[7][1][16] == 0   # FormErr
    assert compiled(nf, [keep('K8S_FlowLayer = "infra"')], k8s_entries=ENTRIES).atoms[0]["truth"] == bytes(3)     # a table without a layer: no key
    # configure: the keep rules first wherever they stand; conditional_sampling: a step per condition, a group per rule
    rm = lambda t, key, **v: dict(type=t, removeEntry=dict(input=key, **v))  # noqa: E731
    t = compiled(nf, [rm("remove_entry_if_exists", "DnsId"), keep("Proto = 6", 10),
                      dict(type="conditional_sampling", conditionalSampling=[dict(value=5, rules=[rm("remove_entry_if_exists", "Bytes"), rm("remove_entry_if_doesnt_exist", "Flags")]),
                                                                              dict(value=0, rules=[])]),
                      dict(type="remove_entry_all_satisfied", removeEntryAllSatisfied=[rm("remove_entry_if_not_equal", "SrcMac", value="00:00:00:00:00:00")]),
                      keep("Proto = 17"), dict(type="conditional_sampling", conditionalSampling=[dict(value=7, rules=[rm("remove_entry_if_exists", "Packets")])])],
                 samplingField="Sampling")
    assert [(s[0], s[1], s[2]) for s in t.steps] == [(0, 0, 10), (0, 0, 0), (1, 0, 0), (2, 0, 5), (2, 0, 0), (1, 0, 0), (2, 1, 7)] and t.flags == F.STORE_SAMPLING
    t = compiled(nf, [dict(type="remove_entry_if_not_equal", removeEntry=dict(input="Sampling", value=2))])   # nothing stores: Sampling stays a uint32
    assert t.atoms == [dict(kind=F.ATOM_PRESENT, field=3)]
    assert nf.TransformFilter('{"rules": []}').steps == [] and nf.TransformFilter(None).steps == []
    nf.Filter(t).close()                                                           # every compiled spec passes the library's checks (no handle)


@pytest.mark.parametrize("cfg, message", [
    (dict(rules=[dict(type="add_field", addField=dict(input="x", value=1))]), "changes fields"),
    (dict(rules=[dict(type="remove_field", removeField=dict(input="Bytes"))]), "changes fields"),
    (dict(rules=[dict(type="add_label_if")]), "changes fields"),
    (dict(rules=[dict(type="add_regex_if")]), "changes fields"),
    (dict(rules=[keep('SrcAddr = "$(DstAddr)"')]), "$(Key) variable"),
    (dict(rules=[keep('Proto =~ "6"')]), "regex on the numeric key"),
    (dict(rules=[keep('SrcAddr =~ "^10"')]), "a regex on 'SrcAddr'"),
    (dict(rules=[keep('AgentIP = "10.0.0.1"')]), "comparison on 'AgentIP'"),
    (dict(rules=[keep("TimeReceived > 5")]), "comparison on 'TimeReceived'"),
    (dict(rules=[keep('Interfaces =~ "eth"')]), "comparison on 'Interfaces'"),
    (dict(rules=[keep("with(_HashId)")]), "'_HashId' is not served"),
    (dict(rules=[keep('_RecordType = "flowLog"')]), "'_RecordType' is not served"),
    (dict(rules=[keep("with(Udns)")]), "'Udns' is not served"),
    (dict(rules=[keep('DnsName =~ "x"')]), "'DnsName' is not served"),
    (dict(rules=[keep('TLSVersion = "TLS 1.3"')]), "'TLSVersion' is not served"),
    (dict(rules=[keep("with(QuicVersion)")]), "'QuicVersion' is not served"),
    (dict(rules=[keep("with(NoSuchKey)")]), "'NoSuchKey' is not served"),
    (dict(rules=[keep('SrcK8S_Name = "a"')]), "needs the Kubernetes table"),
    (dict(rules=[keep('SrcSubnetLabel = "a"')]), "needs the net table"),
    (dict(rules=[keep("Proto = 6")], samplingField="Other"), "only Sampling is served"),
    (dict(rules=[dict(type="remove_entry_if_equal", removeEntry=dict(input="Proto", value=6, castInt=True))]), "castInt"),
    (dict(rules=[dict(type="remove_entry_if_equal", removeEntry=dict(input="FlowDirection", value=1))]), "a number against FlowDirection"),
    (dict(rules=[keep("Proto = 6", 2), dict(type="remove_entry_if_not_equal", removeEntry=dict(input="Sampling", value=2))], samplingField="Sampling"),
     "a number against Sampling"),
    (dict(rules=[dict(type="nonsense")]), "unknown rule type"),
    (dict(rules=[keep("a = 1.5")]), "Float values"),
    (dict(rules=[keep(" or ".join("(Bytes = %d and Packets = %d)" % (k, k) for k in range(33)))]), "more than 64 atoms"),
    (dict(rules=[keep("Proto = %d" % k) for k in range(33)]), "32 steps"),
])
def test_refused_shapes(nf, cfg, message):
    with pytest.raises(ValueError) as e:
        nf.TransformFilter(cfg)
    assert message in str(e.value)


def test_stack_limit(nf):
    deep = lambda d: "Bytes = 0" + "".join(" or (Packets = %d" % k for k in range(d)) + ")" * d  # noqa: E731
    nf.Filter(nf.TransformFilter(dict(rules=[keep(deep(31))]))).close()           # 32 values on the stack
    with pytest.raises(ValueError) as e:
        nf.TransformFilter(dict(rules=[keep(deep(32))]))
    assert "deeper than 32" in str(e.value)


# ---- the roll
def roll_u(seed, idx, step):
    """The documented u over numpy uint64 arrays."""
    def fmix(x):
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xff51afd7ed558ccd)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xc4ceb9fe1a85ec53)
        return x ^ (x >> np.uint64(33))
    k = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        return fmix(fmix(np.uint64(seed) + k * idx) ^ (k * np.uint64(step + 1)))


def test_roll_is_the_same_everywhere(nf):
    rng = np.random.default_rng(7)
    seeds, idx = rng.integers(0, 2**64, 10000, dtype=np.uint64), rng.integers(0, 2**64, 10000, dtype=np.uint64)
    steps, values = rng.integers(0, 32, 10000), rng.integers(0, 65536, 10000)
    values[:100] = 0
    values[100:200] = 1
    for s, i, st, v in zip(seeds.tolist(), idx.tolist(), steps.tolist(), values.tolist()):
        want = FR.roll(s, i, st, v)
        assert nf.filter_roll(s, i, st, v) == want and nf.filter.filter_roll(s, i, st, v) == want
        assert want == (v == 0 or int(roll_u(s, np.uint64(i), st)) % v == 0)


@pytest.mark.parametrize("value", [2, 10, 1000])
def test_roll_is_binomial_within_five_sigma(nf, value):
    """2^20 consecutive indexes: the sampled-in count of binomial(n, 1 / value) lies within five standard deviations of n / value.
    The margin is theory's; three seeds and two steps, so that a lucky constant does not pass."""
    n = 1 << 20
    sigma = math.sqrt(n * (1 / value) * (1 - 1 / value))
    for seed, first, step in ((0, 0, 0), (0x123456789abcdef, 1 << 40, 1), (2**64 - 1, 2**64 - (1 << 19), 31)):
        with np.errstate(over="ignore"):
            idx = np.uint64(first) + np.arange(n, dtype=np.uint64)
        hits = int(np.count_nonzero(roll_u(seed, idx, step) % np.uint64(value) == 0))
        assert abs(hits - n / value) <= 5 * sigma, (value, seed, hits)
        k = 12345
        assert nf.filter_roll(seed, int(idx[k]), step, value) == bool(roll_u(seed, idx[k:k + 1], step)[0] % np.uint64(value) == 0)


# ---- the host side from plain C, and the ABI
def test_filter_host_check_compiles_and_runs(nf, tmp_path):
    lib_dir = os.path.dirname(nf._lib.LIB_PATH)
    exe = str(tmp_path / "filter_host_check")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "c", "filter_host_check.c"),
                           "-o", exe, "-L", lib_dir, "-lnfagg", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "filter host check ok", out.stderr


def test_symbols_layout_and_host_only_filters(nf):
    import ctypes
    L = nf._lib
    for name in ("nfagg_filter_create", "nfagg_filter_destroy", "nfagg_filter_roll", "nfagg_filter_apply", "nfagg_filter_apply_device", "nfagg_gather",
                 "nfagg_gather_device"):
        assert name in L.SIGNATURES and hasattr(L.lib, name)
    assert (ctypes.sizeof(L.FilterAtom), ctypes.sizeof(L.FilterStep), L.FilterAtom.truth.offset, L.FilterAtom.value.offset) == (48, 8, 32, 8)
    assert (L.FILTER_MAX_ATOMS, L.FILTER_MAX_OPS, L.FILTER_MAX_STEPS, L.FILTER_MAX_STACK, L.FILTER_NO_RULE) == (64, 256, 32, 32, 0xFF)
    spec = nf.TransformFilter(dict(rules=[keep('SrcK8S_Name = "a" or DstSubnetLabel = "17"')]), k8s_entries=ENTRIES, labels=LABELS)
    with nf.K8sTable(ENTRIES) as k8s, nf.NetTable(L.NET_SUBNET_LABELS, ([], LABELS), raw=True) as net:
        nf.Filter(spec, k8s, net).close()
        with pytest.raises(nf.NfaggError) as e:
            nf.Filter(spec, k8s, None)
        assert e.value.code == L.EINVAL and "filter atom 1: a subnet-label table atom without a net table" in str(e.value)
        short = nf.TransformFilter(dict(rules=[keep('SrcK8S_Name = "a"')]), k8s_entries=ENTRIES[:2])
        with pytest.raises(nf.NfaggError) as e:
            nf.Filter(short, k8s, net)
        assert "filter atom 0: 3 truth entries, its dimension has 4" in str(e.value)


def test_exporters_want_tls_names_with_a_filter(nf):
    with pytest.raises(ValueError):
        nf.DirectFLPJSON(None, None, filter=object())
    with pytest.raises(ValueError):
        nf.MapTracer(None, 0, 0).evictFlowsJSON(filter=object())
