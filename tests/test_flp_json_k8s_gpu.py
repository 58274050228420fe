"""direct-FLP JSON with Kubernetes enrichment on the GPU (nfagg_encode_flp_json_k8s, nfagg_k8s_resolve; csrc/nfagg_k8s.h,
nfagg_k8s.hip) through the C ABI, host and device entry points, all three policies: every byte and every offset against the
restatement of tests/flp_json_k8s_ref.py, the rows against a Python dict. Records, namer table, parts and network events are
those of the TLS tests; the crafted addresses are found by brute force over the table's hash on the CPU."""
import io
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_k8s_ref as K  # noqa: E402
import flp_json_tls_ref as T  # noqa: E402
import k8s_cases as KC  # noqa: E402
import netev_ref as N  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_flp_json_tls_gpu as TG  # noqa: E402
import test_netev_gpu as E  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, NOW, MONO, RECEIVED, AGENT = G.NAMES, G.NOW, G.MONO, G.RECEIVED, G.AGENT
POLICIES = (0, 1, 2)
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k8s_vectors.json")))
LAYER = (["openshift", "infra-"], [("default", "obj-2"), ("shop", "obj-5")])
# what the informers answer, cycled over a stream's addresses: every gating case, escapes, app and infra namespaces
INFOS = [
    dict(namespace="default", kind="Pod", owner_name="deploy", owner_kind="Deployment", network_name="primary", host_ip="192.168.1.10", host_name="node-1", zone="us-east-1a"),
    dict(kind="Node", owner_kind="Node", network_name="primary", host_ip="192.168.1.11", host_name="node-2", zone=""),
    dict(namespace="default", kind="Service", owner_kind="Service", network_name="primary"),
    dict(namespace="openshift-dns", kind="Pod", network_name="primary", host_ip="fd00::1"),
    dict(namespace="shop", kind="Pod", host_name="orphan-host-name"),
    dict(namespace="shop", kind="Pod", owner_name=b'q"b\\\t\n\r\x01\x7f\xc3\xa9\xff<>&', zone=b"z\x00"),
    dict(),
    dict(namespace="infra-x", kind="Pod", owner_name="o" * 253, network_name="n" * 63, host_name="h" * 253, host_ip="1111:2222:3333:4444:5555:6666:7777:8888", zone="z" * 63),
]


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


def entries_for(recs, every=2):
    """Informer answers for every `every`-th distinct address of the stream's IP records, row k named obj-k."""
    ip = np.isin(recs["metrics"]["eth_protocol"], (0x0800, 0x86DD))
    addrs = sorted({a.tobytes() for a in recs["id"]["src_ip"][ip]} | {a.tobytes() for a in recs["id"]["dst_ip"][ip]})[::every]
    return [(a, dict(INFOS[k % len(INFOS)], name="obj-%d" % k)) for k, a in enumerate(addrs)]


def check(got, want):
    buf, off = got
    wbuf, woff = want
    assert np.asarray(off).astype(np.uint64).tolist() == woff.tolist()
    g = np.asarray(buf).tobytes()
    if g != wbuf:
        gl, wl = g.split(b"\n"), wbuf.split(b"\n")
        k = next(i for i, (a, b) in enumerate(zip(gl, wl)) if a != b)
        raise AssertionError("line %d:\n got %r\nwant %r" % (k, gl[k], wl[k]))


def both_entry_points(nf, tab, tls, k8s, recs, present, parts, ne_table, want_resolve, names=None, agent=AGENT, received=RECEIVED, now=NOW, mono=MONO):
    """The host call and the device call: the size query, a buffer one byte short (NFAGG_TRUNCATED, nothing written), then the
    write into a buffer with canaries behind it. With a network-events table the flows are resolved on the GPU first."""
    import torch
    names = names if names is not None else G.table(nf, NAMES)
    n = len(recs)
    rows = None
    if ne_table is not None:
        present, d_out, rows, missing, _ = tab.netev_resolve(ne_table, present, parts["network_events"], parts["drops"])
        assert set(missing) == want_resolve[4] and rows.tolist() == want_resolve[2].tolist()
        parts = dict(parts, drops=d_out)
    host = tab.encode_flp_json_k8s(recs, tls, k8s, now, mono, names, agent, received, present=present, parts=parts, rows=rows, netev_table=ne_table)
    d_recs = E.dev(recs) if n else None
    d_present = E.dev(present) if present is not None and n else None
    d_parts = {k: E.dev(v) for k, v in (parts or {}).items() if k != "network_events"} if n else {}
    d_rows = E.dev(rows) if rows is not None and n else None
    kw = dict(d_present=d_present.data_ptr() if d_present is not None else 0, d_parts={k: v.data_ptr() for k, v in d_parts.items()},
              d_rows=d_rows.data_ptr() if d_rows is not None else 0, netev_table=ne_table if d_rows is not None else None)
    args = (d_recs.data_ptr() if n else 0, n, tls, k8s, now, mono, names, agent, received)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    rc, need = tab.encode_flp_json_k8s_device(*args, 0, 0, d_off.data_ptr(), **kw)
    assert rc == (nf.TRUNCATED if n else nf.OK) and need == len(host[0])               # the size query: the exact byte count
    d_out = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    if n:
        rc, short = tab.encode_flp_json_k8s_device(*args, d_out.data_ptr(), need - 1, d_off.data_ptr(), **kw)
        torch.cuda.synchronize()
        assert rc == nf.TRUNCATED and short == need and bool((d_out == 0xAB).all())
    rc, wrote = tab.encode_flp_json_k8s_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), **kw)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert rc == nf.OK and wrote == need and (out[need:] == 0xAB).all()
    return host, (out[:need], d_off.cpu().numpy())


def run(nf, tab, tls, tls_ref, entries, layer, recs, present, parts, answers, ne_table):
    events = res = None
    rp, rparts = present, parts
    if answers is not None:
        res = N.resolve(present, parts["network_events"], parts["drops"], answers)
        rp, rparts, events = res[0], dict(parts, drops=res[1]), res[3]
    want = K.encode(recs, tls_ref, K.table_of(entries), layer, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED, present=rp, parts=rparts, events=events)
    with tab.k8s_table(entries, layer) as k8s:
        for got in both_entry_points(nf, tab, tls, k8s, recs, present, parts, ne_table if answers is not None else None, res):
            check(got, want)
    return want


@pytest.fixture(scope="module")
def stream_entries(nf, O):
    return entries_for(TG.policy_inputs(nf, O, 130, 61, 0)[0])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
@pytest.mark.parametrize("policy", POLICIES)
def test_record_counts_policies_and_entry_points(nf, O, tab, go_names, netev_table, stream_entries, policy, n):
    recs, present, parts, answers = TG.policy_inputs(nf, O, 130, 61, policy)
    cut = lambda a: a[:n] if a is not None else None  # noqa: E731
    want = run(nf, tab, go_names[0], go_names[1], stream_entries, LAYER, recs[:n], cut(present), {k: v[:n] for k, v in parts.items()} if parts else parts,
               answers, netev_table)
    assert len(want[1]) == n + 1 and want[0].count(b'"K8S_FlowLayer":"') == n
    if n == 130:
        for text in (b'"K8S_FlowLayer":"app"', b'"K8S_FlowLayer":"infra"', b'"SrcK8S_Zone":""', b'"DstK8S_HostName":"node-1"', b'"DstK8S_Name":"obj-', b'\\u0001'):
            assert text in want[0], text
        if policy == 2:
            assert b'"K8S_FlowLayer":"app","NetworkEvents":[' in want[0] or b'"K8S_FlowLayer":"infra","NetworkEvents":[' in want[0]


@pytest.mark.parametrize("policy", POLICIES)
def test_a_wave_spans_many_windows_and_every_line_is_the_longest(nf, tab, policy):
    """130 flows at the policy's worst case (tests/k8s_cases.py): every line has exactly the bytes the write kernel sizes its
    window by, so the first two waves take a window for every one or two lines and the last wave is partial."""
    n = 130
    case = KC.worst_case(nf, n, policy)
    line, _ = KC.reference({**case, "recs": case["recs"][:1], "present": case["present"][:1] if case["present"] is not None else None,
                            "parts": {k: v[:1] for k, v in case["parts"].items()} if case["parts"] else None})
    max_line = nf._lib.lib.nfagg_flp_json_k8s_max_line(policy)
    window = (32768 - (16 if policy == 0 else 2048) - (max_line + 15) // 16 * 16) // 16 * 16       # FlpK8s<Base>::kWindow
    assert len(line) == max_line and 64 * max_line > 20 * window
    want = (line * n, np.arange(n + 1, dtype=np.uint64) * max_line)                                # every record is the same flow
    ne_table = tab.netev_table(case["answers"].items()) if case["answers"] is not None else None
    res = N.resolve(case["present"], case["parts"]["network_events"], case["parts"]["drops"], case["answers"]) if ne_table is not None else None
    with tab.tls_names(case["tls"]) as tls, tab.k8s_table(case["k8s"], case["layer"]) as k8s:
        for got in both_entry_points(nf, tab, tls, k8s, case["recs"], case["present"], case["parts"], ne_table, res, names=G.table(nf, case["names"]),
                                     agent=case["agent"], received=case["received"], now=case["now"], mono=case["mono"]):
            check(got, want)
    if ne_table is not None:
        ne_table.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_an_empty_table_without_a_layer_gives_the_bytes_of_the_tls_encoder(nf, O, tab, go_names, netev_table, policy):
    recs, present, parts, answers = TG.policy_inputs(nf, O, 300, 67, policy)
    rows = ne = None
    if answers is not None:
        present, d_out, rows, _, _ = tab.netev_resolve(netev_table, present, parts["network_events"], parts["drops"])
        parts, ne = dict(parts, drops=d_out), netev_table
    names = G.table(nf, NAMES)
    old = tab.encode_flp_json_tls(recs, go_names[0], NOW, MONO, names, AGENT, RECEIVED, present=present, parts=parts, rows=rows, netev_table=ne)
    with tab.k8s_table([]) as empty:
        new = tab.encode_flp_json_k8s(recs, go_names[0], empty, NOW, MONO, names, AGENT, RECEIVED, present=present, parts=parts, rows=rows, netev_table=ne)
    assert old[0].tobytes() == new[0].tobytes() and old[1].tolist() == new[1].tolist() and len(old[0]) > 300 * 100


def v6(k: int) -> bytes:
    return bytes.fromhex("20010db8") + int(k).to_bytes(12, "big")


def crafted_family(name):
    """(entries' addresses, addresses to look up that are not in the table)."""
    if name == "one_home":                # 16 rows share one home slot; an absent address walks the whole cluster to the first free slot
        cap = K.capacity(16)
        ips = K.craft(5, cap, 17, v6)
        return ips[:16], ips[16:] + K.craft(4, cap, 1, v6, 10_000) + K.craft(21, cap, 1, v6, 20_000)
    if name == "wrap":                    # the cluster starts three slots before the end of the table and goes on from slot 0
        cap = K.capacity(16)
        ips = K.craft(cap - 3, cap, 17, v6)
        return ips[:16], ips[16:] + K.craft(0, cap, 1, v6, 10_000) + K.craft(cap - 1, cap, 1, v6, 20_000)
    if name == "byte0_byte15":            # keys that differ in their first or in their last byte alone
        base = bytes.fromhex("20010db8000000000000000000000042")
        flip = lambda b, k, x: b[:k] + bytes([b[k] ^ x]) + b[k + 1:]  # noqa: E731
        return [base, flip(base, 0, 1), flip(base, 15, 1), flip(base, 0, 0x80)], [flip(base, 15, 0x80), flip(base, 0, 2), flip(flip(base, 0, 1), 15, 1)]
    if name == "v4_v6_low":               # a v4-mapped and a v6 address with the same last bytes, and the reverse pair absent
        low = bytes([0xff, 0xff, 10, 1, 2, 3])
        return ([bytes(10) + low, bytes.fromhex("20010db8") + bytes(6) + low, bytes.fromhex("fe80") + bytes(10) + bytes([10, 9, 9, 9])],
                [bytes(10) + b"\xff\xff" + bytes([10, 9, 9, 9]), bytes(12) + bytes([10, 1, 2, 3])])
    if name == "one_row":
        return [v6(7)], [v6(8), v6(6), bytes(16)]
    assert name == "half_full"            # 64 rows in 128 slots
    return [v6(k) for k in range(64)], [v6(k) for k in range(64, 80)]


@pytest.mark.parametrize("family", ["one_home", "wrap", "byte0_byte15", "v4_v6_low", "one_row", "half_full"])
def test_lookup_on_crafted_addresses(nf, tab, go_names, family):
    present_ips, absent_ips = crafted_family(family)
    cap = K.capacity(len(present_ips))
    homes = [K.ip_hash(ip) & (cap - 1) for ip in present_ips]
    if family in ("one_home", "wrap"):
        assert len(set(homes)) == 1 and len(present_ips) == 16 and cap == 32 and K.ip_hash(absent_ips[0]) & (cap - 1) == homes[0]
    if family == "half_full":
        assert cap == 2 * len(present_ips)
    entries = [(ip, dict(INFOS[k % len(INFOS)], name="row-%d" % k)) for k, ip in enumerate(present_ips)]
    pool = present_ips + absent_ips
    n = 2 * len(pool) + 2
    recs = np.zeros(n, dtype=nf.FLOW_RECORD)
    recs["metrics"]["eth_protocol"] = np.where(np.arange(n) % 3 == 0, 0x0800, 0x86DD)
    recs["id"]["transport_protocol"] = 6
    for i in range(n):                    # every address on the src side and on the dst side; src == dst on the diagonal
        recs["id"]["src_ip"][i] = np.frombuffer(pool[i % len(pool)], dtype=np.uint8)
        recs["id"]["dst_ip"][i] = np.frombuffer(pool[(i // 2) % len(pool)], dtype=np.uint8)
    assert any(recs["id"]["src_ip"][i].tobytes() == recs["id"]["dst_ip"][i].tobytes() for i in range(n))
    want_rows = K.resolve(recs, entries)
    assert (want_rows != 0xFFFFFFFF).any() and (want_rows == 0xFFFFFFFF).any() and set(range(len(entries))) <= set(want_rows.ravel().tolist())
    want = K.encode(recs, go_names[1], K.table_of(entries), LAYER, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
    with tab.k8s_table(entries, LAYER) as k8s:
        assert tab.k8s_resolve(k8s, recs).tolist() == want_rows.tolist()
        for got in both_entry_points(nf, tab, go_names[0], k8s, recs, None, None, None, None):
            check(got, want)
    for k in range(len(entries)):
        assert b'"SrcK8S_Name":"row-%d"' % k in want[0] and b'"DstK8S_Name":"row-%d"' % k in want[0]


def test_a_record_that_is_not_ip_gets_no_block_and_keeps_its_layer(nf, tab, go_names):
    ip_a, ip_b = bytes(10) + b"\xff\xff" + bytes([10, 0, 0, 1]), v6(1)
    entries = [(ip_a, dict(namespace="shop", name="cart", kind="Pod")), (ip_b, dict(namespace="shop", name="db", kind="Pod"))]
    recs = np.zeros(6, dtype=nf.FLOW_RECORD)
    recs["id"]["src_ip"], recs["id"]["dst_ip"] = np.frombuffer(ip_a, dtype=np.uint8), np.frombuffer(ip_b, dtype=np.uint8)
    recs["metrics"]["eth_protocol"] = [0x0800, 0x0806, 0x86DD, 0, 0x8100, 0x0800]
    want_rows = K.resolve(recs, entries)
    assert want_rows.tolist() == [[0, 1], [0xFFFFFFFF] * 2, [0, 1], [0xFFFFFFFF] * 2, [0xFFFFFFFF] * 2, [0, 1]]
    want = K.encode(recs, go_names[1], K.table_of(entries), LAYER, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
    lines = want[0].split(b"\n")
    assert all(b"K8S_" not in lines[k].replace(b'"K8S_FlowLayer":"infra"', b"") and b'"K8S_FlowLayer":"infra"' in lines[k] for k in (1, 3, 4))
    assert all(b'"K8S_FlowLayer":"app"' in lines[k] and b'"SrcK8S_Name":"cart"' in lines[k] for k in (0, 2, 5))
    with tab.k8s_table(entries, LAYER) as k8s:
        assert tab.k8s_resolve(k8s, recs).tolist() == want_rows.tolist()
        for got in both_entry_points(nf, tab, go_names[0], k8s, recs, None, None, None, None):
            check(got, want)
    want = K.encode(recs, go_names[1], K.table_of(entries), None, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)        # no layer: no key
    assert b"K8S_FlowLayer" not in want[0]
    with tab.k8s_table(entries) as k8s:
        for got in both_entry_points(nf, tab, go_names[0], k8s, recs, None, None, None, None):
            check(got, want)


def test_layer_vectors(nf, tab, go_names):
    """tests/golden/k8s_vectors.json: a prefix match, a ref match, an empty namespace on both sides, app on the dst side only."""
    layer = (GOLDEN["layer"]["prefixes"], [tuple(r) for r in GOLDEN["layer"]["refs"]])
    cases = GOLDEN["layer_cases"]
    recs = np.zeros(len(cases), dtype=nf.FLOW_RECORD)
    recs["metrics"]["eth_protocol"] = 0x0800
    entries = []
    for c, case in enumerate(cases):
        for side, field, last in (("src", "src_ip", 1), ("dst", "dst_ip", 2)):
            ip = bytes(10) + b"\xff\xff" + bytes([10, 1, c, last])
            recs["id"][field][c] = np.frombuffer(ip, dtype=np.uint8)
            if case[side] is not None:
                entries.append((ip, dict(namespace=case[side][0], name=case[side][1], kind="Pod")))
    want = K.encode(recs, go_names[1], K.table_of(entries), layer, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
    for line, case in zip(want[0].split(b"\n"), cases):
        assert b'"K8S_FlowLayer":"%s"' % case["want"].encode() in line, case["name"]
    with tab.k8s_table(entries, layer) as k8s:
        for got in both_entry_points(nf, tab, go_names[0], k8s, recs, None, None, None, None):
            check(got, want)


def test_resolve_against_a_dict_host_and_device(nf, O, tab):
    import torch
    recs = G.stream(nf, O, 5000, seed=71)
    entries = entries_for(recs, every=2)
    want = K.resolve(recs, entries)
    hit = want != 0xFFFFFFFF
    assert len(entries) > 400 and 0.2 < hit.mean() < 0.8 and not hit[recs["metrics"]["eth_protocol"] == 0x0806].any()
    with tab.k8s_table(entries) as k8s:
        assert np.array_equal(tab.k8s_resolve(k8s, recs), want)
        assert tab.k8s_resolve(k8s, recs[:0]).shape == (0, 2)
        d_recs = E.dev(recs)
        d_rows = torch.full((len(recs) + 4, 2), 0x55555555, dtype=torch.int32, device="cuda")
        tab.k8s_resolve_device(k8s, d_recs.data_ptr(), len(recs), d_rows.data_ptr())
        got = d_rows.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:len(recs)], want) and (got[len(recs):] == 0x55555555).all()
    with tab.k8s_table([]) as empty:
        assert (tab.k8s_resolve(empty, recs) == 0xFFFFFFFF).all()


def test_more_than_one_scan_block(nf, O, tab, go_names, netev_table):
    """3000 flows with parts and events: three blocks of the size kernel, 47 waves of the write kernel."""
    recs, present, parts, answers = TG.policy_inputs(nf, O, 3000, 73, 2)
    want = run(nf, tab, go_names[0], go_names[1], entries_for(recs), LAYER, recs, present, parts, answers, netev_table)
    assert want[0].count(b'"SrcK8S_Name"') > 300 and want[0].count(b'"DstK8S_Name"') > 300


def test_argument_checks_with_a_handle(nf, O, tab, go_names):
    recs = G.stream(nf, O, 8, seed=53)
    names = G.table(nf, NAMES)
    with nf.K8sTable([]) as host_only:
        with pytest.raises(nf.NfaggError) as e:
            tab.encode_flp_json_k8s(recs, go_names[0], host_only, NOW, MONO, names, AGENT, RECEIVED)
        assert e.value.code == nf._lib.EINVAL and "Kubernetes table was not created for this handle" in str(e.value)
        with pytest.raises(nf.NfaggError) as e:
            tab.k8s_resolve(host_only, recs)
        assert e.value.code == nf._lib.EINVAL and "Kubernetes table was not created for this handle" in str(e.value)
    with tab.k8s_table([]) as k8s, nf.TlsNames() as host_tls:
        with pytest.raises(nf.NfaggError) as e:
            tab.encode_flp_json_k8s(recs, host_tls, k8s, NOW, MONO, names, AGENT, RECEIVED)
        assert e.value.code == nf._lib.EINVAL and "TLS name table was not created for this handle" in str(e.value)


def test_exporter_and_map_tracer_with_a_table(nf, O, tab, go_names):
    recs = G.stream(nf, O, 700, seed=79, keep_tls=True)
    entries = entries_for(recs)
    out = io.BytesIO()
    with tab.k8s_table(entries, LAYER) as k8s:
        exp = nf.StartDirectFLPJSON(tab, out, names=G.table(nf, NAMES), agent_ip=AGENT, time_received=lambda: RECEIVED, tls_names=go_names[0], k8s=k8s)
        assert exp.ExportEvicted(recs[:400], NOW, MONO) == 400 and exp.ExportEvicted(recs[400:], NOW, MONO) == 300
    want = K.encode(recs, go_names[1], K.table_of(entries), LAYER, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)[0]
    assert out.getvalue() == want and want.count(b'"K8S_FlowLayer"') == 700 and (exp.lines, exp.deferred) == (700, 0)

    from test_map_merge import make_maps
    n_cpu = 4
    main_ids, main_vals, feats = make_maps(O, seed=11, n_pop=400, n_main=300, n_feat=250, n_cpu=n_cpu)
    main_vals["eth_protocol"] = 0x86DD                                        # the maps' random ethertypes would leave no address key
    drained = (main_ids, main_vals, feats, n_cpu)
    decoder = lambda cookie: None if cookie[0] % 2 == 0 else b"event %d" % cookie[1]  # noqa: E731
    mrecs, present, parts, _ = tab.map_merge(main_ids, main_vals, feats, n_cpu)
    entries = entries_for(mrecs)
    (wp, wd, wrows, events, _), answers, _ = N.resolve_loop(present, parts["network_events"], parts["drops"], decoder)
    want = K.encode(mrecs, go_names[1], K.table_of(entries), LAYER, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED, present=wp, parts=dict(parts, drops=wd),
                    events=events)
    mt = nf.MapTracer(nf.GPUMapFetcher(tab, lambda: drained), 0, 0, sample_decoder=decoder, clock=lambda: NOW, mono_clock=lambda: MONO)
    with tab.k8s_table(entries, LAYER) as k8s:
        check(mt.evictFlowsJSON(G.table(nf, NAMES), AGENT, RECEIVED, tls_names=go_names[0], k8s=k8s), want)
    assert any(events) and b'"SrcK8S_Name":"obj-' in want[0] and b'"NetworkEvents":[' in want[0]
