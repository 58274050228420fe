"""direct-FLP JSON with Kubernetes enrichment, CPU side: nfagg_k8s_render against the restatement of
tests/flp_json_k8s_ref.py and the hand-derived vectors of tests/golden/k8s_vectors.json for every gating case; escaping; the
cap at 2048 and 2049 bytes; every error of nfagg_k8s_table_create, each naming its entry; the host-only table; the exported
symbols and struct sizes; the longest lines of the three policies, reached by the restatement; the exporters' argument
rule."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_k8s_ref as K  # noqa: E402
import k8s_cases as KC  # noqa: E402
from flp_json_ref import marshal_sorted  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "k8s_vectors.json")))


def latin(info):
    return {k: None if v is None else v.encode("latin-1") for k, v in info.items()}


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_gating_cases_through_render_restatement_and_vectors(nf, case):
    info = latin(case["info"])
    src = case["src"].encode("latin-1")
    dst = src.replace(b'"SrcK8S_', b'"DstK8S_')
    assert src != dst or src == b""
    for side, want in ((0, src), (1, dst)):
        assert K.render(case["ip"], info, side) == want
        assert nf.k8s_render(case["ip"], info, side) == want


def test_gating_cases_are_all_there():
    names = " / ".join(c["name"] for c in GOLDEN["cases"])
    for text in ("empty namespace", "host IP without host name", "host name without host IP", "zone label with an empty value",
                 "every value empty", "escapes"):
        assert text in names


def test_every_byte_value_escapes_as_jsoniter_does(nf):
    """All 256 byte values in one name: `"` and `\\` with a backslash, \\n \\r \\t, the other bytes below 0x20 as \\u00xx in
    lower-case hex, `<>&` and 0x7f as they are, bytes from 0x80 up copied."""
    info = dict(name=bytes(range(256)), kind=b"<>&", zone=b"\xff\x00")
    got = nf.k8s_render("10.1.2.3", info, 1)
    assert got == K.render("10.1.2.3", info, 1)
    assert b'"DstK8S_Type":"<>&"' in got and b'\\u0000\\u0001' in got and b'\\u001f !\\"#' in got and b"[\\\\]" in got
    assert b"\\t\\n\\u000b\\u000c\\r" in got and bytes(range(0x7f, 0x100)) + b'"' in got and got.endswith(b'"DstK8S_Zone":"\xff\\u0000"')


def test_the_fixed_key_text_is_181_bytes():
    info = {f: b"" for f in K.FIELDS}
    info["host_ip"] = info["host_name"] = info["namespace"] = b"x"           # the three keys an empty value would drop
    assert len(K.render("::1", info, 0)) == KC.KEY_TEXT + 3


@pytest.mark.parametrize("escaped", [False, True])
def test_cap_at_2048_and_2049(nf, escaped):
    ok, over = KC.info_of_block_size(2048, escaped), KC.info_of_block_size(2049, escaped)
    for side in (0, 1):
        assert nf.k8s_render("::1", ok, side) == K.render("::1", ok, side) and len(K.render("::1", ok, side)) == 2048
        with pytest.raises(nf.NfaggError) as e:
            nf.k8s_render("::1", over, side)
        assert e.value.code == nf._lib.EINVAL and "2049 bytes, more than 2048" in str(e.value)
    nf.K8sTable([("::1", ok), ("::2", ok)]).close()
    with pytest.raises(nf.NfaggError) as e:
        nf.K8sTable([("::1", ok), ("::2", over)])
    assert e.value.code == nf._lib.EINVAL and "entry 1: its SrcK8S block has 2049 bytes, the cap is 2048" in str(e.value)
    with pytest.raises(nf.NfaggError) as e:                                  # a value that cannot fit is refused before it is escaped
        nf.K8sTable([("::1", ok), ("::2", ok), ("::3", dict(owner_name=b"\x01" * 2049))])
    assert e.value.code == nf._lib.EINVAL and "entry 2: its SrcK8S block has more than 2048 bytes" in str(e.value)


def test_render_truncated_and_argument_checks(nf):
    L = nf._lib
    e, keep = nf.table._k8s_entry("10.0.0.1", dict(name="a"))
    want = K.render("10.0.0.1", dict(name="a"), 0)
    buf, n = np.full(len(want) + 8, 0xAB, dtype=np.uint8), C.c_size_t(0)
    call = lambda side, cap: L.lib.nfagg_k8s_render(C.byref(e), side, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n))  # noqa: E731
    assert call(0, len(want) - 1) == L.TRUNCATED and n.value == len(want) and (buf == 0xAB).all()
    assert L.lib.nfagg_k8s_render(C.byref(e), 0, None, 0, C.byref(n)) == L.TRUNCATED and n.value == len(want)
    assert call(0, len(want)) == L.OK and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAB).all()
    assert call(2, 64) == L.EINVAL and b"unknown side 2" in L.lib.nfagg_last_error(None)
    assert L.lib.nfagg_k8s_render(None, 0, None, 0, C.byref(n)) == L.EINVAL
    e.name = None                                                            # a length without its string
    assert call(0, 64) == L.EINVAL and b"null string with a length" in L.lib.nfagg_last_error(None)


@pytest.mark.parametrize("entries, message", [
    ([("10.0.0.1", {}), ("10.0.0.2", {}), ("10.0.0.1", {})], "entries 0 and 2 carry the same address"),
    # a v4 entry against its v4-mapped form: the flow id holds both as ::ffff:a.b.c.d
    ([("::1", {}), (bytes([10, 0, 0, 1]), {}), ("::2", {}), (bytes(10) + b"\xff\xff" + bytes([10, 0, 0, 1]), {})], "entries 1 and 3 carry the same address"),
    ([("10.0.0.1", {}), ("::ffff:10.0.0.1", {})], "entries 0 and 1 carry the same address"),
    ([("::1", {}), ("::2", dict(namespace=b"n" * 2049))], "entry 1: its SrcK8S block has more than 2048 bytes"),
    # 102 bytes of key text for the five keys that are always there, 1000 quotes escaped to two bytes each
    ([("::1", dict(zone=b"z" * 1800)), ("::2", {}), ("::3", dict(name=b'"' * 1000))], "entry 2: its SrcK8S block has 2102 bytes, the cap is 2048"),
])
def test_table_errors_name_the_entry(nf, entries, message):
    with pytest.raises(nf.NfaggError) as e:
        nf.K8sTable(entries)
    assert e.value.code == nf._lib.EINVAL and message in str(e.value), str(e.value)


def test_raw_table_errors(nf):
    L = nf._lib
    t = C.c_void_p()
    arr = (L.K8sEntry * 2)()
    arr[1].ip[15] = 1
    arr[1].kind_len = 3                                                      # no pointer behind it
    assert L.lib.nfagg_k8s_table_create(None, arr, 2, None, C.byref(t)) == L.EINVAL and not t.value
    assert b"entry 1: null string with a length" in L.lib.nfagg_last_error(None)
    # one more entry than the table takes: refused before an entry is read
    assert L.lib.nfagg_k8s_table_create(None, arr, L.K8S_MAX_ROWS + 1, None, C.byref(t)) == L.EINVAL and not t.value
    assert b"4194305 Kubernetes entries, more than 4194304" in L.lib.nfagg_last_error(None)
    assert L.lib.nfagg_k8s_table_create(None, None, 1, None, C.byref(t)) == L.EINVAL
    assert L.lib.nfagg_k8s_table_create(None, arr, 1, None, None) == L.EINVAL
    lay = L.K8sLayer(struct_size=8)
    assert L.lib.nfagg_k8s_table_create(None, arr, 1, C.byref(lay), C.byref(t)) == L.EINVAL and b"struct_size" in L.lib.nfagg_last_error(None)
    lay = L.K8sLayer(struct_size=C.sizeof(L.K8sLayer), n_prefixes=1)
    assert L.lib.nfagg_k8s_table_create(None, arr, 1, C.byref(lay), C.byref(t)) == L.EINVAL and b"null layer list" in L.lib.nfagg_last_error(None)


def test_host_only_tables_and_the_empty_table(nf):
    L = nf._lib
    with nf.K8sTable([]) as empty, nf.K8sTable([], ([], [])) as empty_layer:
        assert len(empty) == 0 and not empty.has_layer and empty_layer.has_layer
    entries = [(bytes([10, 0, k >> 8, k & 255]), dict(namespace="ns-%d" % (k % 7), name="pod-%d" % k, kind="Pod")) for k in range(1024)]
    with nf.K8sTable(entries, (["ns-1"], [("ns-2", "pod-2")])) as tab, nf.TlsNames() as tls:
        assert len(tab) == 1024
        o, keep = nf.flp_options(agent_ip=bytes(16))
        off, need = np.zeros(2, dtype=np.uint64), C.c_size_t(7)
        for fn in (L.lib.nfagg_encode_flp_json_k8s, L.lib.nfagg_encode_flp_json_k8s_device):
            # no handle: the call ends at its argument checks, before any device work
            assert fn(None, None, 0, None, None, None, tls._t, tab._t, C.byref(o), None, 0, off.ctypes.data_as(C.c_void_p), C.byref(need)) == L.EINVAL
            assert fn(None, None, 0, None, None, None, tls._t, None, C.byref(o), None, 0, off.ctypes.data_as(C.c_void_p), C.byref(need)) == L.EINVAL
            assert fn(None, None, 0, None, None, None, tls._t, tab._t, None, None, 0, off.ctypes.data_as(C.c_void_p), C.byref(need)) == L.EINVAL
            assert b"null options" in L.lib.nfagg_last_error(None)
        rows = np.zeros(2, dtype=np.uint32)
        for fn in (L.lib.nfagg_k8s_resolve, L.lib.nfagg_k8s_resolve_device):
            assert fn(None, tab._t, None, 0, rows.ctypes.data_as(C.c_void_p)) == L.EINVAL


def test_sizes_and_symbols(nf):
    L = nf._lib
    assert C.sizeof(L.FlpOptions) == 80 and L.lib.nfagg_abi_version() == 2
    assert C.sizeof(L.K8sEntry) == 128 and C.sizeof(L.K8sLayer) == 32 and L.K8sEntry.has_zone.offset == 124 and L.K8sEntry.namespace_len.offset == 88
    assert (L.K8S_MAX_RENDERED, L.K8S_MAX_ROWS, L.K8S_NO_ROW) == (2048, 1 << 22, 0xFFFFFFFF)
    for sym in ("nfagg_k8s_render", "nfagg_k8s_table_create", "nfagg_k8s_table_destroy", "nfagg_k8s_resolve", "nfagg_k8s_resolve_device",
                "nfagg_encode_flp_json_k8s", "nfagg_encode_flp_json_k8s_device", "nfagg_flp_json_k8s_max_line"):
        assert getattr(L.lib, sym) is not None and sym in L.SIGNATURES
    header = open(os.path.join(os.path.dirname(HERE), "include", "nfagg.h")).read()
    for text in ("NFAGG_K8S_MAX_RENDERED 2048", "NFAGG_K8S_MAX_ROWS (1u << 22)", "NFAGG_K8S_NO_ROW 0xFFFFFFFFu", "nfagg_ip_hash(ip, 3)"):
        assert text in header
    assert K.SEED_INDEX == 3 and all(nf.ip_hash(ip, 3) == K.ip_hash(ip) for ip in (bytes(16), bytes(range(16)), b"\xff" * 16))


@pytest.mark.parametrize("policy", [0, 1, 2])
def test_longest_line_is_reached_by_the_restatement(nf, policy):
    """The write kernels size their LDS windows by nfagg_flp_json_k8s_max_line: the longest line without the enrichment, two
    blocks at the cap and the longer layer value. The restatement's line for the worst-case flow has exactly that many bytes,
    and the table takes that flow's row."""
    case = KC.worst_case(nf, 1, policy)
    buf, off = KC.reference(case)
    nf.K8sTable(case["k8s"], case["layer"]).close()
    lib = nf._lib.lib
    assert len(buf) == lib.nfagg_flp_json_k8s_max_line(policy) == lib.nfagg_flp_json_tls_max_line(policy) + 2 * 2048 + len(b',"K8S_FlowLayer":"infra"')
    assert lib.nfagg_flp_json_k8s_max_line(3) == 0 and lib.nfagg_flp_json_k8s_max_line(-1) == 0
    assert buf.count(b'"SrcK8S_') == buf.count(b'"DstK8S_') == 9 and b'"K8S_FlowLayer":"infra"' in buf


@pytest.mark.parametrize("case", GOLDEN["layer_cases"], ids=[c["name"] for c in GOLDEN["layer_cases"]])
def test_layer_vectors_through_the_restatement(case):
    layer = (GOLDEN["layer"]["prefixes"], [tuple(r) for r in GOLDEN["layer"]["refs"]])
    entries, m = [], {}
    for side, ip in (("src", "10.0.0.1"), ("dst", "10.0.0.2")):
        m[b"SrcAddr" if side == "src" else b"DstAddr"] = ip.encode()
        if case[side] is not None:
            entries.append((ip, dict(namespace=case[side][0], name=case[side][1])))
    out = K.add_k8s(m, K.table_of(entries), layer)
    assert out[b"K8S_FlowLayer"] == case["want"].encode()
    assert marshal_sorted(out).count(b"K8S_FlowLayer") == 1
    no_ip = K.add_k8s({b"Etype": 0x0806}, K.table_of(entries), layer)          # EnrichLayer sets the key unconditionally
    assert no_ip == {b"Etype": 0x0806, b"K8S_FlowLayer": b"infra"}


def test_exporters_want_tls_names_with_k8s(nf):
    calls = []

    class Table:
        encode_flp_json = None

        def encode_flp_json_k8s(self, raw, tls_names, k8s, now_ns, mono_ns, names, agent_ip, time_received, unknown):
            calls.append((len(raw), tls_names, k8s, now_ns, mono_ns, time_received))
            return np.frombuffer(b"a\nb\n", dtype=np.uint8), np.array([0, 2, 4], dtype=np.uint64)

    import io
    out = io.BytesIO()
    with pytest.raises(ValueError):
        nf.StartDirectFLPJSON(Table(), out, agent_ip=bytes(16), k8s="table")
    exp = nf.StartDirectFLPJSON(Table(), out, agent_ip=bytes(16), time_received=lambda: 5, tls_names="names", k8s="table")
    assert exp.ExportEvicted(np.zeros(2, dtype=nf.FLOW_RECORD), 11, 13) == 2
    assert calls == [(2, "names", "table", 11, 13, 5)] and out.getvalue() == b"a\nb\n" and (exp.lines, exp.deferred) == (2, 0)
    mt = nf.MapTracer(nf.GPUMapFetcher(None, lambda: None), 0, 0)
    with pytest.raises(ValueError):
        mt.evictFlowsJSON(k8s="table")
