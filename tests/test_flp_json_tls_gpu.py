"""direct-FLP JSON with TLS names on the GPU (nfagg_encode_flp_json_tls, csrc/nfagg_tls.h) through the C ABI, host and device
entry points, all three policies (records only, with the feature parts, with network events as well): every byte and every
offset against the restatement of tests/flp_json_tls_ref.py. The records, namer table, parts and network events are those of
tests/test_flp_json_gpu.py, test_flp_json_content_gpu.py and test_netev_gpu.py."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_tls_ref as T  # noqa: E402
import netev_ref as N  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_netev_gpu as E  # noqa: E402
import tls_worst_case as W  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, NOW, MONO, RECEIVED, AGENT = G.NAMES, G.NOW, G.MONO, G.RECEIVED, G.AGENT
POLICIES = (0, 1, 2)


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


@pytest.fixture(scope="module")
def go_names(nf, tab):
    with tab.tls_names() as t:
        yield t, T.table_of(nf.GO_TLS_NAMES)


@pytest.fixture(scope="module")
def netev_table(tab):
    with tab.netev_table(E.ANSWERS.items()) as t:
        yield t


def check(got, want):
    buf, off = got
    wbuf, woff = want
    assert np.asarray(off).astype(np.uint64).tolist() == woff.tolist()
    assert bytes(np.asarray(buf)) == wbuf


def policy_inputs(nf, O, n, seed, policy):
    """records (their TLS fields as variant 1 sets them), present, parts, the decoder's answers: None where the policy has none."""
    recs, present, parts = E.crafted(nf, O, n, seed)
    if policy == 0:
        return recs, None, None, None
    if policy == 1:
        return recs, present, {k: v for k, v in parts.items() if k != "network_events"}, None
    return recs, present, parts, E.ANSWERS


def both_entry_points(nf, tab, tls, recs, present, parts, ne_table, want_resolve, names=None, agent=AGENT, received=RECEIVED, now=NOW, mono=MONO):
    """The host call and the device call (size query, then the write into a buffer with canaries behind it). With a
    network-events table the flows are resolved on the GPU first, as a caller would."""
    import torch
    names = names if names is not None else G.table(nf, NAMES)
    n = len(recs)
    rows = None
    if ne_table is not None:
        present, d_out, rows, missing, _ = tab.netev_resolve(ne_table, present, parts["network_events"], parts["drops"])
        assert set(missing) == want_resolve[4] and present.tolist() == want_resolve[0].tolist() and rows.tolist() == want_resolve[2].tolist()
        parts = dict(parts, drops=d_out)
    host = tab.encode_flp_json_tls(recs, tls, now, mono, names, agent, received, present=present, parts=parts, rows=rows, netev_table=ne_table)
    d_recs = E.dev(recs) if n else None
    d_present = E.dev(present) if present is not None and n else None
    d_parts = {k: E.dev(v) for k, v in (parts or {}).items() if k != "network_events"} if n else {}
    d_rows = E.dev(rows) if rows is not None and n else None
    kw = dict(d_present=d_present.data_ptr() if d_present is not None else 0, d_parts={k: v.data_ptr() for k, v in d_parts.items()},
              d_rows=d_rows.data_ptr() if d_rows is not None else 0, netev_table=ne_table if d_rows is not None else None)
    args = (d_recs.data_ptr() if n else 0, n, tls, now, mono, names, agent, received)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    rc, need = tab.encode_flp_json_tls_device(*args, 0, 0, d_off.data_ptr(), **kw)
    assert rc == (nf.TRUNCATED if n else nf.OK) and need == len(host[0])               # the size query: the exact byte count
    d_out = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    rc, wrote = tab.encode_flp_json_tls_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), **kw)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert rc == nf.OK and wrote == need and (out[need:] == 0xAB).all()
    return host, (out[:need], d_off.cpu().numpy())


def reference(recs, tls_ref, present, parts, answers, names=NAMES, agent=AGENT, received=RECEIVED, now=NOW, mono=MONO):
    """(the restatement's bytes and offsets, its resolve result or None)."""
    events = res = None
    if answers is not None:
        res = N.resolve(present, parts["network_events"], parts["drops"], answers)
        present, parts, events = res[0], dict(parts, drops=res[1]), res[3]
    return T.encode(recs, tls_ref, now, mono, G.rows(names), agent, received, present=present, parts=parts, events=events), res


def run(nf, tab, tls, tls_ref, recs, present, parts, answers, ne_table):
    want, res = reference(recs, tls_ref, present, parts, answers)
    for got in both_entry_points(nf, tab, tls, recs, present, parts, ne_table if answers is not None else None, res):
        check(got, want)
    return want


def cross_product(nf, O, n):
    """The TLS fields of n records over the whole product of the axes, the address family alternating with it."""
    recs = G.stream(nf, O, n, seed=17)
    versions, flags, ciphers = [0, 0x0303, 0x0304, 0x0200, 0xFFFF], [0, 1], [0, 0x1302, 0xc02f, 0x0001]
    groups, types = [0, 29, 4588, 7, 65535], [0, 0x3f]
    i = np.arange(n)
    m = recs["metrics"]
    m["ssl_version"] = np.array(versions, dtype=np.uint16)[i % 5]
    m["misc_flags"] = np.array(flags, dtype=np.uint8)[(i // 5) % 2] | (m["misc_flags"] & 0xFE)
    m["tls_cipher_suite"] = np.array(ciphers, dtype=np.uint16)[(i // 10) % 4]
    m["tls_key_share"] = np.array(groups, dtype=np.uint16)[(i // 40) % 5]
    m["tls_types"] = np.array(types, dtype=np.uint8)[(i // 200) % 2]
    v6 = (i // 400) % 2 == 1
    m["eth_protocol"] = np.where(v6, 0x86DD, 0x0800)
    recs["id"]["src_ip"][~v6, :12] = recs["id"]["dst_ip"][~v6, :12] = np.frombuffer(bytes(10) + b"\xff\xff", dtype=np.uint8)
    return recs


@pytest.mark.parametrize("policy", POLICIES)
def test_cross_product_of_the_tls_fields(nf, O, tab, go_names, netev_table, policy):
    n = 64 * 9 + 5                                                           # the last wave is partial
    recs = cross_product(nf, O, n)
    _, present, parts, answers = policy_inputs(nf, O, n, 23, policy)
    m = recs["metrics"]
    silent = (m["ssl_version"] == 0) & ((m["misc_flags"] & 1) == 1)
    assert silent.any() and len({(int(a), int(b) & 1, int(c), int(d)) for a, b, c, d in
                                 zip(m["ssl_version"], m["misc_flags"], m["tls_cipher_suite"], m["tls_key_share"])}) == 5 * 2 * 4 * 5
    assert {0x0800, 0x86DD} == set(m["eth_protocol"].tolist()) and {0, 0x3f} == set(m["tls_types"].tolist())
    want = run(nf, tab, go_names[0], go_names[1], recs, present, parts, answers, netev_table)
    lines = want[0].split(b"\n")[:-1]
    assert len(lines) == n and all(b'"TLSVersion"' not in lines[k] for k in np.flatnonzero(silent))
    for text in (b'"TLSVersion":"~ TLS 1.2"', b'"TLSVersion":"0x0200"', b'"TLSVersion":"~ 0xFFFF"', b'"TLSCipherSuite":"0x0001"',
                 b'"TLSCipherSuite":"TLS_ECDHE_RSA_WITH_AES_128_GCM_SHA256"', b'"TLSGroup":"CurveID(7)"', b'"TLSGroup":"CurveID(65535)"',
                 b'"TLSGroup":"X25519MLKEM768","TLSTypes":["ClientHello"', b'"TLSGroup":"X25519","TLSVersion":"TLS 1.3","TimeFlowEndMs"'):
        assert text in want[0], text


TABLE_SHAPES = {
    "empty": [],
    "one_row_per_kind": [(T.VERSION, 0x0303, "v"), (T.CIPHER_SUITE, 0x1302, "c"), (T.GROUP, 29, "g")],
    # 256 rows of one kind, even ids 2..512: the ids looked up below are its first, its last, one in the middle, and absent ones
    # below the first, between two rows and above the last
    "full_versions": [(T.VERSION, 2 * k + 2, "ver-%d" % (2 * k + 2)) for k in range(256)],
    "full_ciphers": [(T.CIPHER_SUITE, 2 * k + 2, "cs-%d" % (2 * k + 2)) for k in range(256)],
    "full_groups": [(T.GROUP, 65535 - 3 * k, "grp-%d" % k) for k in range(256)],
    "name_lengths": [(T.VERSION, 2, "V" * 63), (T.VERSION, 512, "v"), (T.CIPHER_SUITE, 2, "c"), (T.CIPHER_SUITE, 258, "C" * 63),
                     (T.GROUP, 65535, "G" * 63), (T.GROUP, 1, "g")],
}
PROBES = [2, 512, 258, 1, 259, 513, 65535, 65535 - 3 * 255, 65535 - 3 * 128, 65534, 0]


@pytest.mark.parametrize("shape", sorted(TABLE_SHAPES))
def test_table_shapes_and_search_bounds(nf, O, tab, shape):
    n = 3 * len(PROBES) * 2 + 3
    recs = G.stream(nf, O, n, seed=29)
    i = np.arange(n)
    m = recs["metrics"]
    m["ssl_version"] = m["tls_cipher_suite"] = m["tls_key_share"] = 0
    probe = np.array(PROBES, dtype=np.uint16)[(i // 3) % len(PROBES)]
    for k, f in enumerate(("ssl_version", "tls_cipher_suite", "tls_key_share")):
        m[f][i % 3 == k] = probe[i % 3 == k]
    m["ssl_version"][-3:], m["tls_cipher_suite"][-3:], m["tls_key_share"][-3:] = probe[:3], probe[3:6], probe[6:9]      # all three keys on a line
    with tab.tls_names(TABLE_SHAPES[shape]) as tls:
        want = run(nf, tab, tls, T.table_of(TABLE_SHAPES[shape]), recs, None, None, None, None)
    expect = {"empty": b'"TLSVersion":"0x0002"', "one_row_per_kind": b'"TLSGroup":"CurveID(2)"', "full_versions": b'"TLSVersion":"ver-512"',
              "full_ciphers": b'"TLSCipherSuite":"cs-2"', "full_groups": b'"TLSGroup":"grp-255"', "name_lengths": b'"TLSGroup":"' + b"G" * 63 + b'"'}
    assert expect[shape] in want[0]


@pytest.mark.parametrize("policy", POLICIES)
def test_a_wave_spans_several_windows_and_a_line_reaches_the_maximum(nf, tab, policy):
    """128 flows at the policy's worst case (tests/tls_worst_case.py): every wave's 64 lines take several LDS windows, and
    each line has exactly the bytes the write kernel sizes its window by."""
    case = W.worst_case(nf, 128, policy)
    want = W.reference(case)
    lens = np.diff(want[1].astype(np.int64))
    max_line = nf._lib.lib.nfagg_flp_json_tls_max_line(policy)
    window = (32768 - (16 if policy == 0 else 2048) - (max_line + 15) // 16 * 16) // 16 * 16       # FlpTls<Base>::kWindow
    assert lens.max() == max_line and int(lens[:64].sum()) > 2 * window + max_line                 # three windows or more
    ne_table = tab.netev_table(case["answers"].items()) if case["answers"] is not None else None
    res = N.resolve(case["present"], case["parts"]["network_events"], case["parts"]["drops"], case["answers"]) if ne_table is not None else None
    with tab.tls_names(case["tls"]) as tls:
        for got in both_entry_points(nf, tab, tls, case["recs"], case["present"], case["parts"], ne_table, res, names=G.table(nf, case["names"]),
                                     agent=case["agent"], received=case["received"], now=case["now"], mono=case["mono"]):
            check(got, want)
    if ne_table is not None:
        ne_table.close()


def test_agreement_with_the_deferring_encoders_on_one_mixed_stream(nf, O, tab, go_names, netev_table):
    n = 3000
    recs, present, parts = E.crafted(nf, O, n, seed=37)
    m = recs["metrics"]
    has_tls = (m["ssl_version"] != 0) | (m["tls_cipher_suite"] != 0) | (m["tls_key_share"] != 0)
    assert 0.1 * n < has_tls.sum() < 0.9 * n
    names = G.table(nf, NAMES)
    content = {k: v for k, v in parts.items() if k != "network_events"}
    p_out, d_out, rows, missing, _ = tab.netev_resolve(netev_table, present, parts["network_events"], parts["drops"])
    resolved = dict(content, drops=d_out)
    pairs = [(tab.encode_flp_json(recs, NOW, MONO, names, AGENT, RECEIVED),
              tab.encode_flp_json_tls(recs, go_names[0], NOW, MONO, names, AGENT, RECEIVED)),
             (tab.encode_flp_json_content(recs, present, content, NOW, MONO, names, AGENT, RECEIVED),
              tab.encode_flp_json_tls(recs, go_names[0], NOW, MONO, names, AGENT, RECEIVED, present=present, parts=content)),
             (tab.encode_flp_json_netev(recs, p_out, resolved, rows, netev_table, NOW, MONO, names, AGENT, RECEIVED),
              tab.encode_flp_json_tls(recs, go_names[0], NOW, MONO, names, AGENT, RECEIVED, present=p_out, parts=resolved, rows=rows,
                                      netev_table=netev_table))]
    for (old, old_off, deferred), (new, new_off) in pairs:
        assert deferred.astype(bool).tolist() == has_tls.tolist()                     # the old call defers exactly the TLS records
        old, new = old.tobytes(), new.tobytes()
        for i in np.flatnonzero(~has_tls):
            assert old[int(old_off[i]):int(old_off[i + 1])] == new[int(new_off[i]):int(new_off[i + 1])]
        assert all(new_off[i + 1] - new_off[i] > 2 for i in np.flatnonzero(has_tls))
    for f in ("ssl_version", "tls_cipher_suite", "tls_key_share"):
        m[f] = 0
    old = tab.encode_flp_json_content(recs, present, content, NOW, MONO, names, AGENT, RECEIVED)
    new = tab.encode_flp_json_tls(recs, go_names[0], NOW, MONO, names, AGENT, RECEIVED, present=present, parts=content)
    assert old[2].sum() == 0 and old[0].tobytes() == new[0].tobytes() and old[1].tolist() == new[1].tolist()
    old = tab.encode_flp_json(recs, NOW, MONO, names, AGENT, RECEIVED)
    new = tab.encode_flp_json_tls(recs, go_names[0], NOW, MONO, names, AGENT, RECEIVED)
    assert old[0].tobytes() == new[0].tobytes() and old[1].tolist() == new[1].tolist()


def test_more_than_one_scan_block_of_blocks(nf, O, tab, go_names):
    """66 000 records: 65 blocks of the size kernel, more than the 64 the scan of the block sums takes at once."""
    recs = G.stream(nf, O, 66_000, seed=41, keep_tls=True)
    assert (recs["metrics"]["ssl_version"] != 0).sum() > 1000
    run(nf, tab, go_names[0], go_names[1], recs, None, None, None, None)


@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("policy", POLICIES)
def test_edges(nf, O, tab, go_names, netev_table, policy, n):
    recs, present, parts, answers = policy_inputs(nf, O, max(n, 1), 43, policy)
    cut = lambda a: a[:n] if a is not None else None  # noqa: E731
    recs["metrics"]["ssl_version"], recs["metrics"]["misc_flags"] = 0x0303, 1
    want = run(nf, tab, go_names[0], go_names[1], recs[:n], cut(present), {k: v[:n] for k, v in parts.items()} if parts else parts, answers, netev_table)
    assert len(want[1]) == n + 1 and (n == 0 or b'"TLSVersion":"~ TLS 1.2"' in want[0])


def test_one_byte_short_writes_nothing(nf, O, tab, go_names):
    import ctypes as C
    import torch
    n = 300
    recs = G.stream(nf, O, n, seed=47, keep_tls=True)
    names = G.table(nf, NAMES)
    want, want_off = T.encode(recs, go_names[1], NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
    o, keep = nf.flp_options(NOW, MONO, names, AGENT, RECEIVED)
    need = C.c_size_t(0)
    small = np.full(len(want) - 1, 0xAB, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    rc = nf._lib.lib.nfagg_encode_flp_json_tls(tab._h, recs.ctypes.data_as(C.c_void_p), n, None, None, None, go_names[0]._t, C.byref(o),
                                               small.ctypes.data_as(C.c_void_p), len(small), off.ctypes.data_as(C.c_void_p), C.byref(need))
    assert rc == nf.TRUNCATED and need.value == len(want) and (small == 0xAB).all() and not off.any()
    d_recs = E.dev(recs)
    d_out = torch.full((len(want) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    args = (d_recs.data_ptr(), n, go_names[0], NOW, MONO, names, AGENT, RECEIVED)
    rc, got = tab.encode_flp_json_tls_device(*args, d_out.data_ptr(), len(want) - 1, d_off.data_ptr())
    torch.cuda.synchronize()
    assert rc == nf.TRUNCATED and got == len(want) and (d_out.cpu().numpy() == 0xAB).all() and not d_off.cpu().numpy().any()
    rc, got = tab.encode_flp_json_tls_device(*args, d_out.data_ptr(), len(want), d_off.data_ptr())
    torch.cuda.synchronize()
    assert rc == nf.OK and got == len(want) and (d_out.cpu().numpy()[len(want):] == 0xAB).all()
    check((d_out.cpu().numpy()[:len(want)], d_off.cpu().numpy()), (want, want_off))


def test_argument_checks_with_a_handle(nf, O, tab, go_names, netev_table):
    recs = G.stream(nf, O, 8, seed=53)
    names = G.table(nf, NAMES)
    rows = np.full((8, 4), 0xFFFF, dtype=np.uint16)
    present = np.zeros(8, dtype=np.uint8)
    with nf.TlsNames() as host_only:
        with pytest.raises(nf.NfaggError) as e:
            tab.encode_flp_json_tls(recs, host_only, NOW, MONO, names, AGENT, RECEIVED)
        assert e.value.code == nf._lib.EINVAL and "was not created for this handle" in str(e.value)
    with pytest.raises(nf.NfaggError) as e:                                   # rows without their table
        tab.encode_flp_json_tls(recs, go_names[0], NOW, MONO, names, AGENT, RECEIVED, present=present, parts={}, rows=rows)
    assert e.value.code == nf._lib.EINVAL and "go together" in str(e.value)


def test_exporter_with_a_table_over_a_stream_half_tls(nf, O, tab, go_names):
    recs = G.stream(nf, O, 2000, seed=59, keep_tls=True)
    half = np.arange(len(recs)) % 2 == 0
    for f in ("ssl_version", "tls_cipher_suite", "tls_key_share"):
        recs["metrics"][f][~half] = 0
    recs["metrics"]["ssl_version"][half] |= 0x0300
    calls, writes = [], []

    class Stream(io.BytesIO):
        def write(self, b):
            writes.append(len(b))
            return super().write(b)

    out = Stream()
    exp = nf.StartDirectFLPJSON(tab, out, names=G.table(nf, NAMES), agent_ip=AGENT, time_received=lambda: RECEIVED,
                                fallback=lambda *a: calls.append(a) or b"", tls_names=go_names[0])
    assert exp.ExportEvicted(recs[:1200], NOW, MONO) == 1200 and exp.ExportEvicted(recs[1200:], NOW, MONO) == 800
    want = T.encode(recs, go_names[1], NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)[0]
    assert calls == [] and len(writes) == 2 and out.getvalue() == want and want.count(b'"TLSVersion"') == 1000 and (exp.lines, exp.deferred) == (2000, 0)


def test_map_tracer_with_a_table(nf, O, tab, go_names):
    """MapTracer.evictFlowsJSON(tls_names=...) on a small drained map with parts, events and TLS."""
    from test_map_merge import make_maps
    n_cpu = 4
    main_ids, main_vals, feats = make_maps(O, seed=11, n_pop=400, n_main=300, n_feat=250, n_cpu=n_cpu)
    main_vals["misc_flags"][::3] |= 1

    def decoder(cookie):
        if cookie[0] % 4 == 0:
            return None
        if cookie[0] % 4 == 1:
            return b"event %d" % cookie[1]
        return ("drop" if cookie[0] % 4 == 2 else "allow", "NetpolNode", "n", "", "Ingress", b"acl %d" % (cookie[1] % 3))

    drained = (main_ids, main_vals, feats, n_cpu)
    mt = nf.MapTracer(nf.GPUMapFetcher(tab, lambda: drained), 0, 0, sample_decoder=decoder, clock=lambda: NOW, mono_clock=lambda: MONO)
    got = mt.evictFlowsJSON(G.table(nf, NAMES), AGENT, RECEIVED, tls_names=go_names[0])
    recs, present, parts, _ = tab.map_merge(main_ids, main_vals, feats, n_cpu)
    (wp, wd, wrows, events, _), answers, _ = N.resolve_loop(present, parts["network_events"], parts["drops"], decoder)
    m = recs["metrics"]
    assert ((m["ssl_version"] != 0) | (m["tls_cipher_suite"] != 0) | (m["tls_key_share"] != 0)).sum() > 50 and any(events) and len(got) == 2
    want = T.encode(recs, go_names[1], NOW, MONO, G.rows(NAMES), AGENT, RECEIVED, present=wp, parts=dict(parts, drops=wd), events=events)
    check(got, want)
    assert b'"NetworkEvents":[' in want[0] and b'"TLSVersion":"~ ' in want[0]
    mt2 = nf.MapTracer(nf.GPUMapFetcher(tab, lambda: drained), 0, 0, clock=lambda: NOW, mono_clock=lambda: MONO)      # no decoder: the content policy
    check(mt2.evictFlowsJSON(G.table(nf, NAMES), AGENT, RECEIVED, tls_names=go_names[0]),
          T.encode(recs, go_names[1], NOW, MONO, G.rows(NAMES), AGENT, RECEIVED, present=present, parts=parts))
