"""direct-FLP JSON with TLS names, CPU side: the reference's own TLS vectors (tests/golden/tls_vectors.json) through
nfagg_tls_names_render and through the restatement of tests/flp_json_tls_ref.py; the fall-back formats; every error of
nfagg_tls_names_create, each naming its entry; the host-only table; GO_TLS_NAMES against tests/ref_decode.py; the options'
size and the exported symbols; the longest lines of the three policies, reached by the restatement; the exporter's
bookkeeping with a table."""
import ctypes as C
import io
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_tls_ref as T  # noqa: E402
import ref_decode  # noqa: E402
import tls_worst_case as W  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "tls_vectors.json")))
KEYS = (("TLSVersion", "ssl_version", T.VERSION), ("TLSCipherSuite", "tls_cipher_suite", T.CIPHER_SUITE), ("TLSGroup", "tls_key_share", T.GROUP))


def test_reference_vectors_through_render_and_restatement(nf):
    entries = [tuple(e) for e in GOLDEN["names"]]
    ref = T.table_of(entries)
    assert len(GOLDEN["vectors"]) == 5
    with nf.TlsNames(entries) as tab:
        for v in GOLDEN["vectors"]:
            rec = np.zeros(1, dtype=nf.FLOW_RECORD)
            for f in ("ssl_version", "tls_cipher_suite", "tls_key_share", "misc_flags"):
                rec["metrics"][f] = v[f]
            m = T.add_tls({}, rec.tobytes(), ref)
            for key, field, kind in KEYS:
                want = v[key]
                assert (m.get(key.encode()).decode() if key.encode() in m else None) == want, (v["source"], key)
                if want is not None:
                    assert tab.render(kind, v[field], bool(v["misc_flags"] & 1)) == want.encode(), (v["source"], key)


def test_fall_back_formats(nf):
    with nf.TlsNames([]) as empty, nf.TlsNames() as go:
        assert len(empty) == 0 and len(go) == len(nf.GO_TLS_NAMES)
        for tab in (empty, go):
            for ident, text in ((0x0001, b"0x0001"), (0x0200, b"0x0200"), (0x0A0B, b"0x0A0B"), (0xFFFF, b"0xFFFF")):
                for kind in (T.VERSION, T.CIPHER_SUITE):
                    assert tab.render(kind, ident) == text == T.render({}, kind, ident)
                assert tab.render(T.VERSION, ident, True) == b"~ " + text == T.render({}, T.VERSION, ident, True)
                assert tab.render(T.CIPHER_SUITE, ident, True) == text                 # the flag belongs to the version alone
            for ident, text in ((1, b"CurveID(1)"), (9, b"CurveID(9)"), (10, b"CurveID(10)"), (65535, b"CurveID(65535)")):
                assert tab.render(T.GROUP, ident) == text == T.render({}, T.GROUP, ident)
                assert tab.render(T.GROUP, ident, True) == text
            with pytest.raises(ValueError):                                            # 99999 does not fit the record's uint16
                tab.render(T.GROUP, 99999)
            with pytest.raises(ValueError):
                T.render({}, T.GROUP, 99999)
        with pytest.raises(ValueError):
            nf.TlsNames([(T.GROUP, 99999, "x")])
        assert go.render(T.VERSION, 0x0304) == b"TLS 1.3" and go.render(T.GROUP, 4588) == b"X25519MLKEM768"
        assert go.render(T.CIPHER_SUITE, 0xc02f) == b"TLS_ECDHE_RSA_WITH_AES_128_GCM_SHA256"


def test_render_truncated_and_argument_checks(nf):
    L = nf._lib
    with nf.TlsNames([(T.VERSION, 0x0303, "TLS 1.2")]) as tab:
        buf, n = np.full(16, 0xAB, dtype=np.uint8), C.c_size_t(0)
        call = lambda kind, cap: L.lib.nfagg_tls_names_render(tab._t, kind, 0x0303, 1, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n))  # noqa: E731
        assert call(T.VERSION, 8) == L.TRUNCATED and n.value == 9 and (buf == 0xAB).all()
        assert L.lib.nfagg_tls_names_render(tab._t, T.VERSION, 0x0303, 1, None, 0, C.byref(n)) == L.TRUNCATED and n.value == 9
        assert call(T.VERSION, 9) == L.OK and buf[:9].tobytes() == b"~ TLS 1.2" and (buf[9:] == 0xAB).all()
        assert call(3, 16) == L.EINVAL and b"unknown kind 3" in L.lib.nfagg_last_error(None)
        assert L.lib.nfagg_tls_names_render(None, 0, 1, 0, None, 0, C.byref(n)) == L.EINVAL


@pytest.mark.parametrize("entries, message", [
    ([(0, 1, "a"), (3, 1, "b")], b"entry 1: unknown kind 3"),
    ([(0, 1, "a"), (1, 1, "b"), (0, 1, "c")], b"entries 0 and 2 carry the same kind 0 and id 0x0001"),
    ([(2, 7, "g"), (2, 8, "")], b"entry 1: empty name"),
    ([(1, 5, "x" * 63), (1, 6, "x" * 64)], b"entry 1: a name of 64 bytes"),
    ([(2, k, "n%d" % k) for k in range(257)], b"entry 256: more than 256 rows of kind 2"),
    ([(0, 1, "ok"), (0, 2, 'q"')], b"entry 1: byte 0x22 at 1"),
    ([(0, 2, "b\\")], b"entry 0: byte 0x5c at 1"),
    ([(1, 2, "ab"), (1, 3, "a\x1fb")], b"entry 1: byte 0x1f at 1"),
    ([(1, 3, b"\x00")], b"entry 0: byte 0x00 at 0"),
])
def test_table_errors_name_the_entry(nf, entries, message):
    with pytest.raises(nf.NfaggError) as e:
        nf.TlsNames(entries)
    assert e.value.code == nf._lib.EINVAL and message in str(e.value).encode(), str(e.value)


def test_table_limits_are_accepted(nf):
    rows = [(k, i, "x" * 63 if i % 2 else "y") for k in range(3) for i in range(256)]
    with nf.TlsNames(rows) as tab:
        assert tab.render(T.GROUP, 255) == b"x" * 63 and tab.render(T.VERSION, 254) == b"y" and tab.render(T.CIPHER_SUITE, 256) == b"0x0100"
    with nf.TlsNames([(T.VERSION, 5, b"\x7f\x80\xff caf\xc3\xa9")]) as tab:     # what WriteString copies as it is
        assert tab.render(T.VERSION, 5, True) == b"~ \x7f\x80\xff caf\xc3\xa9"


def test_host_only_table_renders_and_is_refused_by_the_encoders(nf):
    L = nf._lib
    with nf.TlsNames() as tab:
        assert tab.render(T.VERSION, 0x0303) == b"TLS 1.2"
        o, keep = nf.flp_options(agent_ip=bytes(16))
        off, need = np.zeros(2, dtype=np.uint64), C.c_size_t(7)
        for fn in (L.lib.nfagg_encode_flp_json_tls, L.lib.nfagg_encode_flp_json_tls_device):
            # no handle here either: the call ends at its argument checks, before any device work
            assert fn(None, None, 0, None, None, None, tab._t, C.byref(o), None, 0, off.ctypes.data_as(C.c_void_p), C.byref(need)) == L.EINVAL
            assert fn(None, None, 0, None, None, None, None, C.byref(o), None, 0, off.ctypes.data_as(C.c_void_p), C.byref(need)) == L.EINVAL
            assert fn(None, None, 0, None, None, None, tab._t, None, None, 0, off.ctypes.data_as(C.c_void_p), C.byref(need)) == L.EINVAL
            assert b"null options" in L.lib.nfagg_last_error(None)


def test_go_tls_names_equal_the_decode_restatement(nf):
    want = ([(T.VERSION, i, n) for i, n in ref_decode.TLS_VERSIONS.items()] + [(T.CIPHER_SUITE, i, n) for i, n in ref_decode.CIPHER_SUITES.items()] +
            [(T.GROUP, i, n) for i, n in ref_decode.CURVES.items()])
    assert sorted(nf.GO_TLS_NAMES) == sorted(want) and len(set((k, i) for k, i, _ in nf.GO_TLS_NAMES)) == len(want)
    assert (nf._lib.TLS_VERSION, nf._lib.TLS_CIPHER_SUITE, nf._lib.TLS_GROUP) == (T.VERSION, T.CIPHER_SUITE, T.GROUP)


def test_options_size_unchanged_and_symbols_exported(nf):
    assert C.sizeof(nf._lib.FlpOptions) == 80 and nf._lib.lib.nfagg_abi_version() == 2
    assert C.sizeof(nf._lib.TlsNameEntry) == 16 and (nf._lib.TLS_NAME_MAX, nf._lib.TLS_MAX_ROWS) == (63, 256)
    for sym in ("nfagg_tls_names_create", "nfagg_tls_names_destroy", "nfagg_tls_names_render", "nfagg_encode_flp_json_tls",
                "nfagg_encode_flp_json_tls_device", "nfagg_flp_json_tls_max_line"):
        assert getattr(nf._lib.lib, sym) is not None and sym in nf._lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(HERE), "include", "nfagg.h")).read()
    for text in ("NFAGG_TLS_NAME_MAX 63", "NFAGG_TLS_MAX_ROWS 256", "NFAGG_TLS_VERSION = 0", "NFAGG_TLS_CIPHER_SUITE = 1", "NFAGG_TLS_GROUP = 2"):
        assert text in header


@pytest.mark.parametrize("policy", [0, 1, 2])
def test_longest_line_is_reached_by_the_restatement(nf, policy):
    """The write kernels size their LDS windows by nfagg_flp_json_tls_max_line; the restatement's line for the worst-case
    flow of tests/tls_worst_case.py has exactly that many bytes (and the key-by-key argument that none is longer is in
    DESIGN.md §4.7f)."""
    case = W.worst_case(nf, 1, policy)
    buf, off = W.reference(case)
    if case["answers"] is not None:                      # the events fit the cap of both renderings: the table takes them
        nf.NetevTable(case["answers"].items()).close()
    assert len(buf) == nf._lib.lib.nfagg_flp_json_tls_max_line(policy) > 4088 and nf._lib.lib.nfagg_flp_json_tls_max_line(3) == 0


def test_exporter_with_a_table_never_calls_fallback(nf):
    """DirectFLPJSON(tls_names=...): one write per eviction from encode_flp_json_tls, whatever the records carry."""
    calls = []

    class Table:
        encode_flp_json = None

        def encode_flp_json_tls(self, raw, tls_names, now_ns, mono_ns, names, agent_ip, time_received, unknown):
            calls.append((len(raw), tls_names, now_ns, mono_ns, time_received))
            buf = b"".join(b"L%d\n" % int(r["id"]["src_port"]) for r in raw)
            return np.frombuffer(buf, dtype=np.uint8), np.cumsum([0] + [len(b"L%d\n" % int(r["id"]["src_port"])) for r in raw]).astype(np.uint64)

    recs = np.zeros(5, dtype=nf.FLOW_RECORD)
    recs["id"]["src_port"] = np.arange(5) + 7
    recs["metrics"]["ssl_version"][[1, 3]] = 0x0304

    def fallback(*a):
        raise AssertionError("fallback called")

    writes = []
    out = io.BytesIO()
    out.write = lambda b, w=out.write: (writes.append(bytes(b)), w(b))[1]
    exp = nf.StartDirectFLPJSON(Table(), out, agent_ip=bytes(16), time_received=lambda: 5, fallback=fallback, tls_names="names")
    assert exp.ExportEvicted(recs, 11, 13) == 5 and exp.ExportEvicted(recs[:0], 11, 13) == 0
    assert calls == [(5, "names", 11, 13, 5)] and writes == [b"L7\nL8\nL9\nL10\nL11\n"] and (exp.lines, exp.deferred) == (5, 0)
