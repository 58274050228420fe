"""write loki on the device, CPU side: the restatement of tests/loki_ref.py pinned against hand-derived bytes and a protobuf
decode, LabelSet.String() against literal expectations, the timestamp arithmetic against integers, the Python compiler's
refusals, the C spec checks and the table built without a handle."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loki_ref as LR  # noqa: E402


# ---- a decoder that knows nothing of the restatement: google.protobuf over a descriptor built from the field numbers of
# pkg/logproto/types.go:88-144 and timestamp.go:59-106
def _messages():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    f = descriptor_pb2.FileDescriptorProto(name="loki_test.proto", package="lokitest", syntax="proto3")
    T = descriptor_pb2.FieldDescriptorProto

    def msg(name, fields):
        m = f.message_type.add(name=name)
        for fname, num, typ, label, tname in fields:
            m.field.add(name=fname, number=num, type=typ, label=label, type_name=tname)
    msg("Timestamp", [("seconds", 1, T.TYPE_INT64, T.LABEL_OPTIONAL, None), ("nanos", 2, T.TYPE_INT32, T.LABEL_OPTIONAL, None)])
    msg("Entry", [("timestamp", 1, T.TYPE_MESSAGE, T.LABEL_OPTIONAL, ".lokitest.Timestamp"), ("line", 2, T.TYPE_BYTES, T.LABEL_OPTIONAL, None)])
    msg("Stream", [("labels", 1, T.TYPE_BYTES, T.LABEL_OPTIONAL, None), ("entries", 2, T.TYPE_MESSAGE, T.LABEL_REPEATED, ".lokitest.Entry")])
    msg("PushRequest", [("streams", 1, T.TYPE_MESSAGE, T.LABEL_REPEATED, ".lokitest.Stream")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(f)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("lokitest.PushRequest"))


_PUSH = None


def decode_push_request(body: bytes):
    """[(labels, [(seconds, nanos, line)])] of one body."""
    global _PUSH
    _PUSH = _PUSH or _messages()
    req = _PUSH()
    req.ParseFromString(bytes(body))
    return [(bytes(s.labels), [(e.timestamp.seconds, e.timestamp.nanos, bytes(e.line)) for e in s.entries]) for s in req.streams]


def test_one_entry_by_hand():
    """types.go:88-144: 0a <stream>; stream = 0a <labels> 12 <entry>; entry = 0a <timestamp> 12 <line>; timestamp = 08 <seconds> 10 <nanos>."""
    line, labels = b'{"a":1}', b'{x="y"}'
    ts = bytes([0x08, 0x05, 0x10, 0x07])                                              # 5 s, 7 ns
    entry = bytes([0x0A, 4]) + ts + bytes([0x12, 7]) + line
    stream = bytes([0x0A, 7]) + labels + bytes([0x12, len(entry)]) + entry
    want = bytes([0x0A, len(stream)]) + stream
    assert LR.marshal_push_request([(labels, [(5, 7, line)])]) == want
    assert decode_push_request(want) == [(labels, [(5, 7, line)])]


def test_two_entries_two_streams_and_the_empty_timestamp_by_hand():
    """An entry's timestamp field is always there, with length 0 for the zero time; a negative second takes ten bytes."""
    e0 = bytes([0x0A, 0, 0x12, 2]) + b"{}"                                            # seconds 0, nanos 0
    e1 = bytes([0x0A, 11, 0x08]) + b"\xff" * 9 + b"\x01" + bytes([0x12, 2]) + b"{}"   # seconds -1
    s0 = bytes([0x0A, 2]) + b"{}" + bytes([0x12, len(e0)]) + e0 + bytes([0x12, len(e1)]) + e1
    e2 = bytes([0x0A, 6, 0x10, 0xFF, 0x93, 0xEB, 0xDC, 0x03, 0x12, 1]) + b"x"         # nanos 999 999 999
    s1 = bytes([0x0A, 5]) + b'{a=1}' + bytes([0x12, len(e2)]) + e2
    want = bytes([0x0A, len(s0)]) + s0 + bytes([0x0A, len(s1)]) + s1
    got = LR.marshal_push_request([(b"{}", [(0, 0, b"{}"), (-1, 0, b"{}")]), (b"{a=1}", [(0, 999999999, b"x")])])
    assert got == want
    assert decode_push_request(got) == [(b"{}", [(0, 0, b"{}"), (-1, 0, b"{}")]), (b"{a=1}", [(0, 999999999, b"x")])]


@pytest.mark.parametrize("n", [127, 128, 16383, 16384])
def test_varint_edges_decode(n):
    body = LR.marshal_push_request([(b"{}", [(1, 0, b"l" * n)])])
    assert decode_push_request(body) == [(b"{}", [(1, 0, b"l" * n)])]


def test_labelset_string_literals(nf):
    """labelset_string.go:23-43: {a="..", b=".."}, names sorted, strconv.AppendQuote."""
    cases = [({}, b"{}"),
             ({"app": "flows"}, b'{app="flows"}'),
             ({"b": "2", "a": "1", "_c": ""}, b'{_c="", a="1", b="2"}'),
             ({"k": b'q"\\'}, b'{k="q\\"\\\\"}'),
             ({"k": b"\a\b\f\n\r\t\v"}, b'{k="\\a\\b\\f\\n\\r\\t\\v"}'),
             ({"k": b"\x00\x01\x1f\x7f ~"}, b'{k="\\x00\\x01\\x1f\\x7f ~"}')]
    for labels, want in cases:
        assert nf.labelset_string(labels) == want
        assert LR.labelset_string({LR._b(k): LR._b(v) for k, v in labels.items()}) == want
    with pytest.raises(ValueError):
        nf.labelset_string({"k": "é"})


def _exact_timestamp(ms: int, scale: int):
    """float64(ms) * float64(scale) rounded to nearest, ties to even, by integer arithmetic alone; then Go's truncating / and %
    and time.Unix's normalisation."""
    p = ms * scale
    a = abs(p)
    if a >= 1 << 53:
        shift = a.bit_length() - 53
        q, rem = a >> shift, a & ((1 << shift) - 1)
        half = 1 << (shift - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
        a = q << shift
    p = a if p >= 0 else -a
    if not (-(1 << 63) <= p < 1 << 63):
        return None
    sec = abs(p) // 10 ** 9 * (1 if p >= 0 else -1)
    nsec = p - sec * 10 ** 9
    if nsec < 0:
        sec, nsec = sec - 1, nsec + 10 ** 9
    return sec, nsec


TS_CASES = [1, 999, 1000, 1001, 1760000000000, 1760000000001, 1760000000123, -1, -1500, -1000,
            (1 << 53) // 10 ** 6 + 1, 9007199254741, 9007199254743,          # products beyond 2^53: rounding
            253402300799999, 253402300800000,                                  # the last valid second, year 10000
            9223372036854, 9223372036855, -9223372036855]                      # around the int64 edge


@pytest.mark.parametrize("ms", TS_CASES)
def test_timestamp_against_integer_arithmetic(nf, ms):
    want = _exact_timestamp(ms, 10 ** 6)
    assert LR.extract_timestamp({b"TimeFlowEndMs": ms}, b"TimeFlowEndMs", 1e6, 5) == want
    assert nf.loki.extract_timestamp(ms, 1e6, 5) == want


def test_timestamp_ties_round_to_even():
    """ms * 15625 (a scale of 15.625 us) lands exactly half way between two float64 values for these ms."""
    found = 0
    for ms in range((1 << 53) // 15625 + 1, (1 << 53) // 15625 + 4000):
        p = ms * 15625
        if p >= 1 << 53 and p % 2 == 1 and p < 1 << 54:                       # spacing 2: an odd product is a tie
            want = _exact_timestamp(ms, 15625)
            assert Fraction(want[0] * 10 ** 9 + want[1]) in (Fraction(p - 1), Fraction(p + 1)) and (want[0] * 10 ** 9 + want[1]) % 4 == 0
            assert LR.extract_timestamp({b"T": ms}, b"T", 15625.0, 0) == want
            found += 1
    assert found > 100


def test_timestamp_zero_missing_and_now():
    assert LR.extract_timestamp({b"T": 0}, b"T", 1e6, 1500000000123456789) == (1500000000, 123456789)
    assert LR.extract_timestamp({}, b"T", 1e6, -1) == (-1, 999999999)
    assert LR.extract_timestamp({b"T": 7}, b"", 1e6, 2 * 10 ** 9) == (2, 0)


def test_cut_rule_is_strictly_greater():
    maps = [{b"k": b"v" * 10}] * 4                                                    # a line is {"k":"vvvvvvvvvv"}: 18 bytes
    n_line = len(LR.marshal_sorted(maps[0]))
    for size, want in ((1, [1, 1, 1, 1]), (2 * n_line, [2, 2]), (2 * n_line - 1, [1, 1, 1, 1]), (3 * n_line, [3, 1]), (4 * n_line, [4])):
        bodies, batches, deferred = LR.write_loki(maps, {}, (), {}, "", 1.0, size, 10 ** 9)
        assert [sum(len(e) for _, e in b) for b in batches] == want and not deferred


def test_split_labels_lines_rules():
    m = {b"a": b"x", b"b": 2, b"c": b"\xff", b"d": b"", b"e": b"keep"}
    labels, lines = LR.split_labels_lines(m, {b"a": "A", b"b": "B", b"c": "C", b"d": "D", b"zz": "Z"}, {b"e"}, {"s": "t"})
    assert labels == {b"s": b"t", b"A": b"x", b"B": b"2", b"D": b""} and lines == {}      # invalid UTF-8: gone from both; "" is a value


# ---- the Python compiler
def test_write_loki_defaults_and_masks(nf):
    L = nf._lib
    w = nf.WriteLoki({})
    assert (w.batch_size, w.batch_wait, w.timeout, w.max_retries, w.timestamp_label, w.timestamp_scale, w.format) == (102400, "1s", "10s", 10, "TimeReceived", 1e9, "json")
    w = nf.WriteLoki(dict(labels=["SrcK8S_Namespace", "DstK8S_OwnerName", "K8S_FlowLayer", "FlowDirection", "_RecordType", "9bad"], ignoreList=["SrcK8S_Zone", "_HashId"],
                          timestampLabel="TimeFlowEndMs", timestampScale="1ms", batchSize=10 << 20, staticLabels={"app": "netobserv-flowcollector"}))
    assert w.label_keys == L.DIM_SRC_K8S(0) | L.DIM_DST_K8S(3) | L.DIM_FLOW_LAYER | L.DIM_FLOW_DIRECTION | L.LOKI_KEY_RECORD_TYPE
    assert w.ignore_keys == L.DIM_SRC_K8S(8) | L.LOKI_KEY_HASH_ID and w.timestamp_source == L.LOKI_TS_TIME_FLOW_END_MS and w.timestamp_scale == 1e6
    assert "9bad" not in w.sane_labels                                                # LegacyValidation drops it at construction
    assert nf.loki.sanitize("a/b.c-d") == "a_b_c_d"
    assert [nf.loki.parse_duration(t) for t in ("1s", "1ms", "1.5us", "1h2m", "15625ns")] == [10 ** 9, 10 ** 6, 1500, 3720 * 10 ** 9, 15625]


@pytest.mark.parametrize("config", [dict(labels=["Proto"]), dict(ignoreList=["Interfaces"]), dict(labels=["Dscp"]), dict(labels=["_HashId"]), dict(format="printf"),
                                    dict(timestampLabel="Bytes"), dict(ignoreList=["TimeFlowEndMs"], timestampLabel="TimeFlowEndMs"), dict(batchSize=1 << 31),
                                    dict(timestampScale="0s"), dict(clientProtocol="udp")])
def test_write_loki_refuses_what_is_not_served(nf, config):
    with pytest.raises(ValueError):
        nf.WriteLoki(config)


# ---- the C ABI without a device
ENTRIES = [("10.0.0.1", dict(namespace="shop", name="a", kind="Pod", owner_name="cart", owner_kind="Deployment", host_ip="192.168.1.10", host_name="n1", zone="z")),
           ("10.0.0.2", dict(namespace="shop", name="b", kind="Pod", owner_name="cart", owner_kind="Deployment")),
           ("10.0.0.3", dict(namespace="", name="c", kind="Node", owner_name="", owner_kind="Node")),
           ("10.0.0.4", dict(namespace="shop", name="d", kind="Pod", owner_name=b"bad\xff", owner_kind="Deployment")),
           ("10.0.0.5", dict(name="e"))]
OPERATOR = ["SrcK8S_Namespace", "SrcK8S_OwnerName", "SrcK8S_OwnerType", "DstK8S_Namespace", "DstK8S_OwnerName", "DstK8S_OwnerType", "K8S_FlowLayer", "FlowDirection",
            "_RecordType"]


def host_tables(nf, labels=OPERATOR, ignore=(), cats=(("lan", ["10.0.0.0/8"]), ("", ["11.0.0.0/8"]), ("lan", ["12.0.0.0/8"]), (b"x\xff", ["13.0.0.0/8"]))):
    k8s = nf.K8sTable(ENTRIES, None, None)
    net = nf.NetTable(nf._lib.NET_SUBNET_LABELS, cats, None)
    w = nf.WriteLoki(dict(labels=list(labels), ignoreList=list(ignore), timestampLabel="TimeFlowEndMs", timestampScale="1ms"))
    return k8s, net, w


def test_host_only_table_classes_and_blocks(nf):
    k8s, net, w = host_tables(nf)
    with nf.LokiTable(w, k8s, net) as t:
        # rows 0 and 1 share (shop, cart, Deployment); row 2: namespace absent, owner name "" present; row 3: its owner name is not
        # valid UTF-8 and counts as absent; row 4: only the always-present empty fields
        assert t.n_classes(0) == 4 and t.n_classes(1) == 4
        assert [t.class_row(0, c) for c in (1, 2, 3, 4)] == [0, 2, 3, 4]
        assert t.render(0, 0) == b',"SrcK8S_HostIP":"192.168.1.10","SrcK8S_HostName":"n1","SrcK8S_Name":"a","SrcK8S_NetworkName":"","SrcK8S_Type":"Pod","SrcK8S_Zone":"z"'
        assert t.render(1, 2) == b',"DstK8S_Name":"c","DstK8S_NetworkName":"","DstK8S_Type":"Node"'
        assert b"OwnerName" not in t.render(0, 3) and b"bad" not in t.render(0, 3)          # gone from the line as well
        with pytest.raises(nf.NfaggError):
            t.class_row(0, 5)
    # nothing masked: the blocks are the Kubernetes table's own
    with nf.LokiTable(nf.WriteLoki(dict(timestampLabel="TimeFlowEndMs")), k8s, net) as t:
        assert t.n_classes(0) == 0 and t.render(0, 3) == nf.k8s_render("10.0.0.4", ENTRIES[3][1], 0)
    # ignored and label together: ignored wins, no class
    with nf.LokiTable(nf.WriteLoki(dict(labels=["SrcK8S_Name"], ignoreList=["SrcK8S_Name"], timestampLabel="TimeFlowEndMs")), k8s, net) as t:
        assert t.n_classes(0) == 0 and b"SrcK8S_Name\"" not in t.render(0, 0)


def test_spec_refusals_through_the_c_abi(nf):
    L = nf._lib
    k8s, net, w = host_tables(nf)
    good = w.spec()
    bad = []
    for field, value, text in (("struct_size", 8, "struct_size"), ("label_keys", L.DIM_PROTO, "label_keys: unknown key bits 0x400000"),
                               ("ignore_keys", 1 << 25, "ignore_keys: unknown key bits 0x2000000"), ("label_keys", L.LOKI_KEY_HASH_ID, "_HashId as a label"),
                               ("timestamp_source", 3, "unknown timestamp source 3"), ("timestamp_scale", 0.0, "timestamp_scale"),
                               ("timestamp_scale", float("inf"), "timestamp_scale"), ("timestamp_scale", float("nan"), "timestamp_scale"),
                               ("batch_size", 0, "batch_size 0"), ("batch_size", 1 << 31, "batch_size")):
        s = L.LokiSpec.from_buffer_copy(good)
        setattr(s, field, value)
        with pytest.raises(nf.NfaggError) as e:
            nf.LokiTable(w, k8s, net, spec=s)
        assert text in str(e.value)
        bad.append(text)
    assert len(bad) == 10
    out = C.c_void_p()
    assert L.lib.nfagg_loki_table_create(None, None, net._t, C.byref(good), C.byref(out)) == L.EINVAL
    assert L.lib.nfagg_loki_table_create(None, k8s._t, net._t, None, C.byref(out)) == L.EINVAL
    assert L.lib.nfagg_loki_table_create(None, k8s._t, net._t, C.byref(good), None) == L.EINVAL


def test_loki_host_check_compiles_and_runs(nf, tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(nf._lib.LIB_PATH)
    exe = str(tmp_path / "loki_host_check")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tools", "c", "loki_host_check.c"),
                           "-o", exe, "-L", lib_dir, "-lnfagg", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "loki host check ok", out.stderr


def test_symbols_signatures_and_sizes(nf):
    L = nf._lib
    for sym in ("nfagg_loki_table_create", "nfagg_loki_table_destroy", "nfagg_loki_n_classes", "nfagg_loki_class_row", "nfagg_loki_render", "nfagg_loki_plan",
                "nfagg_loki_plan_device", "nfagg_loki_write", "nfagg_loki_write_device", "nfagg_loki_max_entry"):
        assert sym in L.SIGNATURES and getattr(L.lib, sym)
    assert L.SIGNATURES["nfagg_loki_plan"] == L.SIGNATURES["nfagg_loki_plan_device"] and L.SIGNATURES["nfagg_loki_write"] == L.SIGNATURES["nfagg_loki_write_device"]
    assert C.sizeof(L.LokiSpec) == 32 and C.sizeof(L.LokiCounts) == 16 and nf.LOKI_STREAM.itemsize == 20 and nf.LOKI_GROUP.itemsize == 24
    assert [L.lib.nfagg_loki_max_entry(p) for p in range(4)] == [L.lib.nfagg_flp_json_conn_max_line(p) - 1 + 27 for p in range(3)] + [0]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nfagg.h")).read()
    for sym in L.SIGNATURES:
        if sym.startswith("nfagg_loki_"):
            assert sym + "(" in header
