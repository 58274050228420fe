"""Network events on the device path (csrc/nfagg_netev.hip, the *_netev instantiations of csrc/nfagg_pb.hip and
csrc/nfagg_flp_content.hip) against the restatement of tests/netev_ref.py, byte for byte, through the host and the device
entry points: the reference's two known answers, crafted flows at the sizes where the two-pass skeleton turns, tables on both
sides of the LDS staging threshold, the missing-cookie set, waves whose lines all carry four events rendered at the cap, the
equivalence with the *_content entry points when no flow has an event, and the MapTracer mirror with a Python decoder."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netev_ref as N  # noqa: E402
import pb_window_mixes as W  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
from test_flp_json_content_gpu import content_parts  # noqa: E402
from test_netev_cpu import VEC, fake_decoder, kat_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, NOW, MONO, RECEIVED, AGENT = G.NAMES, G.NOW, G.MONO, G.RECEIVED, G.AGENT
PB_NAMES = [(i, m, n if isinstance(n, str) else "esc", u if isinstance(u, str) else "udn") for (i, m, n, u) in NAMES]   # the oracle's table takes str
LDS_ROWS = 256                                             # kNetevLdsRows (csrc/nfagg_netev.hip)


def ck(k: int) -> bytes:
    return int(k).to_bytes(8, "little")


S_ALLOW = "Allowed by network policy p in namespace ns, direction Ingress"
S_DROP = "Dropped by network policy p in namespace ns, direction Ingress"
ALLOW, ALLOW_REL, DROP, DROP_BOGUS, MSG, MSG_DROP, UNDEC, ZERO = ck(11), ck(0xFFFFFFFFFFFFFFFF), ck(5), ck(1 << 63), ck(77), ck(78), ck(300), ck(0)
MISSING1, MISSING2 = ck(0xABCDEF0123), ck(9)
ANSWERS = {
    ALLOW: ("allow", "NetworkPolicy", "p", "ns", "Ingress", S_ALLOW),
    ALLOW_REL: ("allow-related", "NetworkPolicy", "p", "ns", "Ingress", S_ALLOW),      # same String(), another map
    DROP: ("drop", "NetworkPolicy", "p", "ns", "Ingress", S_DROP),
    DROP_BOGUS: ("drop", "NoSuchActor", 'q"\\\n\x01\xff', "", "Egress", S_DROP),      # same String() as DROP, unknown actor: cause + 0
    MSG: b"sampled by something that is no ACL",
    MSG_DROP: b"drop",                                                                 # a non-ACL event named "drop": no injection
    UNDEC: None,
    ZERO: ("drop", "UDNIsolation", "", "", "", "Dropped by UDN isolation of type "),
}
# (cookies, packets, bytes) of the crafted flows; flow i takes pattern i % len(PATTERNS)
PATTERNS = [
    ([ALLOW, DROP, ALLOW_REL, DROP_BOGUS], [1, 2, 3, 4], [10, 20, 30, 40]),        # four slots; first map wins; seen drop still injects
    ([DROP, ALLOW, DROP, MSG_DROP], [3, 0, 65535, 1], [65000, 9, 65535, 1]),        # a packets == 0 slot between; saturation
    ([UNDEC, MISSING1, ZERO, ALLOW], [1, 1, 1, 1], [1, 2, 3, 4]),
    ([MISSING2, MISSING1, ALLOW, ALLOW], [5, 6, 7, 8], [0, 0, 0, 0]),
    ([DROP, DROP, DROP, DROP], [0, 0, 0, 0], [1, 1, 1, 1]),                        # nothing counted
    ([MSG, MSG_DROP, DROP_BOGUS, ALLOW_REL], [1, 1, 65535, 1], [1, 1, 65535, 1]),
    ([ZERO, ZERO, MSG, UNDEC], [2, 2, 0, 2], [100, 100, 100, 100]),
]


def crafted(nf, O, n, seed, answers=ANSWERS):
    """records (every third keeps its TLS words: deferred), present, parts (the five content parts and network_events)."""
    recs = G.stream(nf, O, n, seed=seed, keep_tls=True)
    present, parts = content_parts(nf, n, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    ne = np.zeros(n, dtype=nf.NETWORK_EVENTS)
    ne.view(np.uint8).reshape(n, 72)[:] = rng.integers(0, 256, (n, 72), dtype=np.uint8)
    for i in range(n):
        c, pk, by = PATTERNS[i % len(PATTERNS)]
        ne["network_events"][i] = np.frombuffer(b"".join(c), dtype=np.uint8).reshape(4, 8)
        ne["packets"][i], ne["bytes"][i] = pk, by
    idx = np.arange(n)
    present[idx % 8 != 7] |= N.FEAT_NETEV
    present[idx % 8 == 7] &= ~np.uint8(N.FEAT_NETEV)
    present[idx % 5 == 0] = 63                                                         # every part: both neighbours of the key
    recs["metrics"]["packets"][idx % 5 == 0] = 7
    d = parts["drops"]
    d["bytes"][idx % 4 == 1] = 65530                                                   # an existing part that saturates
    d["packets"][idx % 4 == 1] = 65535
    parts = dict(parts, network_events=ne)
    return recs, present, parts


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host_resolve(tab, table, present, parts, missing_cap=64, drops=True):
    p, d, rows, missing, over = tab.netev_resolve(table, present, parts.get("network_events"), parts["drops"] if drops else None, missing_cap)
    return p, d.view(np.uint8).reshape(len(p), 32), rows, set(missing), over


def device_resolve(tab, table, present, parts, missing_cap=64, drops=True, in_place=False):
    import torch
    n = len(present)
    d_p, d_ne = dev(present), dev(parts["network_events"])
    d_d = dev(parts["drops"]) if drops else None
    d_po = d_p if in_place else torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    d_do = d_d if in_place and drops else torch.full((n * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    d_rows = torch.full((n * 4,), 0x7777, dtype=torch.int16, device="cuda")
    d_set = torch.full((max(missing_cap, 1),), -1, dtype=torch.int64, device="cuda")
    n_miss, zero, over = tab.netev_resolve_device(table, d_p.data_ptr(), d_ne.data_ptr(), d_d.data_ptr() if drops else 0, n, d_po.data_ptr(),
                                                  d_do.data_ptr(), d_rows.data_ptr(), d_set.data_ptr() if missing_cap else 0, missing_cap)
    torch.cuda.synchronize()
    slots = d_set.cpu().numpy().view(np.uint64)[:missing_cap]
    missing = [ck(v) for v in slots[slots != 0]] + ([ZERO] if zero else [])
    assert len(missing) == len(set(missing)) == n_miss
    return (d_po.cpu().numpy(), d_do.cpu().numpy().reshape(n, 32), d_rows.cpu().numpy().view(np.uint16).reshape(n, 4), set(missing), over), \
        (d_po, d_do, d_rows)


def check_resolve(got, want):
    p, d, rows, missing, over = got
    wp, wd, wrows, _, wmissing = want
    assert np.array_equal(p, wp), np.flatnonzero(p != wp)[:5]
    assert np.array_equal(rows, wrows), np.flatnonzero((rows != wrows).any(axis=1))[:5]
    assert np.array_equal(d, wd), np.flatnonzero((d != wd).any(axis=1))[:5]
    assert missing == wmissing and not over


def device_encode_json(nf, tab, table, recs, p_out, parts, d_rows_np):
    import torch
    n = len(recs)
    d_recs, d_present, d_rows = dev(recs), dev(p_out), dev(d_rows_np)
    d_parts = {k: dev(v) for k, v in parts.items() if k != "network_events"}
    ptrs = {k: v.data_ptr() for k, v in d_parts.items()}
    args = (d_recs.data_ptr(), n, d_present.data_ptr(), ptrs, d_rows.data_ptr(), table, NOW, MONO, G.table(nf, NAMES), AGENT, RECEIVED)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_def = torch.full((n,), 0xCD, dtype=torch.uint8, device="cuda")
    rc, need, _ = tab.encode_flp_json_netev_device(*args, 0, 0, d_off.data_ptr())
    assert rc == nf.TRUNCATED
    d_out = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    rc, wrote, n_def = tab.encode_flp_json_netev_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), d_def.data_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert rc == nf.OK and wrote == need and (out[need:] == 0xAB).all()
    return out[:need], d_off.cpu().numpy(), d_def.cpu().numpy()


def device_encode_pb(nf, tab, table, recs, p_out, parts, d_rows_np):
    import torch
    n = len(recs)
    d_recs, d_present, d_rows = dev(recs), dev(p_out), dev(d_rows_np)
    d_parts = {k: dev(v) for k, v in parts.items() if k != "network_events"}
    ptrs = {k: v.data_ptr() for k, v in d_parts.items()}
    args = (d_recs.data_ptr(), n, d_present.data_ptr(), ptrs, d_rows.data_ptr(), table, NOW, MONO, AGENT, nf.intf_table(PB_NAMES))
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_len = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc, need = tab.encode_pb_netev_device(*args, 0, 0, d_off.data_ptr(), d_len.data_ptr())
    assert rc == nf.TRUNCATED
    d_out = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    rc, wrote = tab.encode_pb_netev_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), d_len.data_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert rc == nf.OK and wrote == need and (out[need:] == 0xAB).all()
    return out[:need], d_off.cpu().numpy(), d_len.cpu().numpy().view(np.uint32)


def check_pb(got, want):
    buf, off, blen = got
    wbuf, woff, wlen = want
    assert np.asarray(off).astype(np.uint64).tolist() == woff.tolist()
    assert np.asarray(blen).tolist() == wlen.tolist()
    g = np.asarray(buf).tobytes()
    if g != wbuf:
        k = next(i for i in range(len(wlen)) if g[int(woff[i]):int(woff[i + 1])] != wbuf[int(woff[i]):int(woff[i + 1])])
        raise AssertionError("frame %d:\n got %s\nwant %s" % (k, g[int(woff[k]):int(woff[k + 1])].hex(), wbuf[int(woff[k]):int(woff[k + 1])].hex()))


def check_all(nf, O, tab, table, answers, recs, present, parts, json_too=True, pb_too=True, drops=True):
    """Resolve and both encoders, host and device entry points, against the restatement."""
    want = N.resolve(present, parts["network_events"], parts["drops"] if drops else None, answers)
    wp, wd, wrows, events, _ = want
    check_resolve(host_resolve(tab, table, present, parts, drops=drops), want)
    got, _ = device_resolve(tab, table, present, parts, drops=drops)
    check_resolve(got, want)
    dparts = {k: v for k, v in parts.items() if k != "network_events"}
    dparts["drops"] = wd.copy().view(nf.PKT_DROP).reshape(-1)
    if json_too:
        wj = N.encode_json(recs, wp, dparts, events, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
        G.check(tab.encode_flp_json_netev(recs, wp, dparts, wrows, table, NOW, MONO, G.table(nf, NAMES), AGENT, RECEIVED), wj)
        G.check(device_encode_json(nf, tab, table, recs, wp, dparts, wrows), wj)
    if pb_too:
        wpb = N.encode_pb(O, recs, wp, dparts, events, NOW, MONO, AGENT, PB_NAMES)
        check_pb(tab.encode_pb_netev(recs, wp, dparts, wrows, table, NOW, MONO, AGENT, nf.intf_table(PB_NAMES)), wpb)
        check_pb(device_encode_pb(nf, tab, table, recs, wp, dparts, wrows), wpb)
    return want


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


@pytest.fixture(scope="module")
def table(tab):
    with tab.netev_table(ANSWERS.items()) as t:
        yield t


@pytest.mark.parametrize("case", VEC["cases"], ids=[c["name"] for c in VEC["cases"]])
def test_reference_kats(nf, O, tab, case):
    present, ne, drops = kat_inputs(O, case)
    answers = {bytes.fromhex(c): fake_decoder(bytes.fromhex(c)) for c in case["network_events"]["cookies"][:2]}
    recs = G.stream(nf, O, 1, seed=3)
    parts = {"network_events": ne.view(nf.NETWORK_EVENTS), "drops": (drops if drops is not None else np.zeros(1, dtype=O.DROPS)).view(nf.PKT_DROP)}
    with tab.netev_table(answers.items()) as t:
        wp, wd, wrows, events, _ = check_all(nf, O, tab, t, answers, recs, present, parts, drops=drops is not None)
    d = wd.view(O.DROPS).reshape(-1)[0]
    assert {k: int(d[k]) for k in case["expect_drops"]} == case["expect_drops"] and len(events[0]) == 2


@pytest.mark.parametrize("n", [1, 64, 65, 1024, 1025])
def test_crafted_flows_at_the_skeleton_sizes(nf, O, tab, table, n):
    recs, present, parts = crafted(nf, O, n, seed=40 + n)
    wp, wd, wrows, events, missing = check_all(nf, O, tab, table, ANSWERS, recs, present, parts)
    if n >= 64:
        assert missing == {MISSING1, MISSING2}
        assert any(len(e) == 4 for e in events) and (wrows[:, 0] == N.NO_ROW).any()
        d = wd.view(O.DROPS).reshape(-1)
        assert (d["bytes"] == 65535).any() and (d["latest_drop_cause"] == 1 << 24).any() and (d["latest_drop_cause"] == (1 << 24) + 9).any()
        assert ((wp & N.FEAT_DROPS) != 0).sum() > ((present & N.FEAT_DROPS) != 0).sum()


def test_no_drops_array_at_all(nf, O, tab, table):
    """drops == NULL: no flow has the part whatever present says; an injected drop still gets its part and its bit."""
    recs, present, parts = crafted(nf, O, 130, seed=7)
    wp, wd, _, _, _ = check_all(nf, O, tab, table, ANSWERS, recs, present, parts, drops=False)
    has = (wp & N.FEAT_DROPS) != 0
    assert has.any() and not has.all() and not wd[~has].any()


def test_in_place_outputs(nf, O, tab, table):
    recs, present, parts = crafted(nf, O, 300, seed=8)
    want = N.resolve(present, parts["network_events"], parts["drops"], ANSWERS)
    got, _ = device_resolve(tab, table, present, parts, in_place=True)
    check_resolve(got, want)


@pytest.mark.parametrize("rows", [0, 1, 2, LDS_ROWS, LDS_ROWS + 1, 1500])
def test_table_sizes_around_the_lds_threshold(nf, O, tab, rows):
    rng = np.random.default_rng(rows)
    cookies = [ck(v) for v in rng.integers(1, 2**63, rows + 40, dtype=np.uint64)]
    kinds = [("drop", "EgressFirewall", "n%d" % k, "ns", "Egress", "s%d" % (k // 2)) if k % 3 == 0 else b"message %d" % (k // 3) if k % 3 == 1 else None
             for k in range(rows)]
    answers = dict(zip(cookies[:rows], kinds))
    n = 200
    recs = G.stream(nf, O, n, seed=rows + 1)
    present, parts = content_parts(nf, n, seed=rows + 2)
    present |= N.FEAT_NETEV
    ne = np.zeros(n, dtype=nf.NETWORK_EVENTS)
    pick = rng.integers(0, len(cookies), (n, 4))
    ne["network_events"] = np.frombuffer(b"".join(cookies), dtype=np.uint8).reshape(-1, 8)[pick]
    ne["packets"], ne["bytes"] = rng.integers(0, 3, (n, 4)), rng.integers(0, 70000, (n, 4)) & 0xFFFF
    parts = dict(parts, network_events=ne)
    with tab.netev_table(answers.items()) as t:
        assert len(t) == rows
        want = check_all(nf, O, tab, t, answers, recs, present, parts, pb_too=rows in (2, LDS_ROWS + 1))
    assert want[4] and (rows < 2 or (want[2] != N.NO_ROW).any())


def test_missing_set_capacities_and_the_loop(nf, O, tab):
    rng = np.random.default_rng(5)
    n, distinct = 3000, 150
    cookies = [ZERO] + [ck(v) for v in rng.integers(1, 2**64 - 1, distinct - 1, dtype=np.uint64)]
    recs = G.stream(nf, O, n, seed=5)
    present = np.full(n, N.FEAT_NETEV, dtype=np.uint8)
    ne = np.zeros(n, dtype=nf.NETWORK_EVENTS)
    ne["network_events"] = np.frombuffer(b"".join(cookies), dtype=np.uint8).reshape(-1, 8)[rng.integers(0, distinct, (n, 4))]
    ne["packets"] = 1
    parts = {"network_events": ne, "drops": np.zeros(n, dtype=nf.PKT_DROP)}
    assert {bytes(c) for c in ne["network_events"].reshape(-1, 8)} == set(cookies)
    with tab.netev_table([]) as empty:
        for cap in (distinct, distinct + 1, 4096):                                  # holds them all (the zero cookie takes no slot)
            for got in (host_resolve(tab, empty, present, parts, cap), device_resolve(tab, empty, present, parts, cap)[0]):
                assert got[3] == set(cookies) and not got[4] and not (got[2] != N.NO_ROW).any()
        for cap in (0, 1, 40, distinct - 2):                                        # too small: a subset, no duplicates, the flag
            for got in (host_resolve(tab, empty, present, parts, cap), device_resolve(tab, empty, present, parts, cap)[0]):
                assert got[4] and got[3] < set(cookies) and len(got[3]) >= min(cap, 1)
    # the loop of the protocol with a set that is too small for one round: it converges to the full result
    decoder = lambda c: None if c[1] % 5 == 0 else ("drop", "MulticastNS", "n", "ns", "", b"s" + c[:1])
    answers, calls = {}, 0
    while True:
        with tab.netev_table(answers.items()) as t:
            got = host_resolve(tab, t, present, parts, 64)
        if not got[3]:
            break
        for c in got[3]:
            answers[c] = decoder(c)
            calls += 1
    assert calls == distinct == len(answers)
    want = N.resolve(present, ne, parts["drops"], answers)
    check_resolve(got, want)


def capped_events(k):
    """Four events whose JSON object and protobuf message both have exactly 512 bytes, with four different String()s."""
    return [b'"' + bytes([97 + k % 26, 97 + j]) + b"m" * 494 for j in range(4)]


@pytest.mark.parametrize("n", [64, 1024 + 64, 1024 + 64 + 37])
def test_waves_of_lines_with_four_events_at_the_cap(nf, O, tab, n):
    """Every flow carries four events rendered at the cap: each wave of the JSON write kernel walks several windows — the first
    wave, the first wave of the second scan block, the ragged last wave; the protobuf frames run through the 24 KiB window."""
    answers = {}
    recs = G.stream(nf, O, n, seed=n)
    present, parts = content_parts(nf, n, seed=n + 1)
    present |= N.FEAT_NETEV
    ne = np.zeros(n, dtype=nf.NETWORK_EVENTS)
    ne["packets"] = 1
    for i in range(n):
        for j, ev in enumerate(capped_events(i % 5)):
            c = ck(1000 + 4 * (i % 5) + j)
            answers[c] = ev
            ne["network_events"][i, j] = np.frombuffer(c, dtype=np.uint8)
    for ev in answers.values():
        assert len(N.render_json(ev)) == 512 == len(N.render_pb(ev))
    parts = dict(parts, network_events=ne)
    with tab.netev_table(answers.items()) as t:
        wp, wd, wrows, events, _ = check_all(nf, O, tab, t, answers, recs, present, parts)
    assert all(len(e) == 4 for e in events)


@pytest.mark.parametrize("window, n", [(8192, 24_000), (16384, 4_000)])
def test_capped_wave_under_the_smaller_protobuf_windows(nf, O, tab, window, n):
    """One wave of 64 flows with four events at the cap among plain flows: the call's average frame length picks the 8 KiB or
    the 16 KiB instantiation of the protobuf write kernel, and that wave spans many of its windows."""
    # plain Accounter records average 108 bytes a frame, the scrambled stream 187: with the 64 long frames, 114 and 219
    recs = O.gen_stream(n, seed=window, n_keys=997, variant=0).view(nf.FLOW_RECORD) if window == 8192 else G.stream(nf, O, n, seed=window)
    present = np.zeros(n, dtype=np.uint8)
    parts = {"drops": np.zeros(n, dtype=nf.PKT_DROP), "network_events": np.zeros(n, dtype=nf.NETWORK_EVENTS)}
    answers = {ck(1000 + j): ev for j, ev in enumerate(capped_events(0))}
    at = 1024 + 128 + 5                                                              # not wave-aligned: two waves carry them
    present[at:at + 64] = N.FEAT_NETEV
    parts["network_events"]["packets"][at:at + 64] = 1
    parts["network_events"]["network_events"][at:at + 64] = np.frombuffer(b"".join(answers), dtype=np.uint8).reshape(4, 8)
    with tab.netev_table(answers.items()) as t:
        want = N.resolve(present, parts["network_events"], parts["drops"], answers)
        wpb = N.encode_pb(O, recs, want[0], {"drops": parts["drops"]}, want[3], NOW, MONO, AGENT, PB_NAMES)
        assert W.window_for(np.diff(wpb[1].astype(np.int64))) == window
        check_pb(tab.encode_pb_netev(recs, want[0], {"drops": parts["drops"]}, want[2], t, NOW, MONO, AGENT, nf.intf_table(PB_NAMES)), wpb)


def test_empty_table_and_no_rows_equal_the_content_encoders(nf, O, tab):
    n = 2000
    recs = G.stream(nf, O, n, seed=31, keep_tls=True)
    present, parts = content_parts(nf, n, seed=32)
    rows = np.full((n, 4), N.NO_ROW, dtype=np.uint16)
    names = G.table(nf, NAMES)
    with tab.netev_table([]) as empty:
        j = a = tab.encode_flp_json_netev(recs, present, parts, rows, empty, NOW, MONO, names, AGENT, RECEIVED)
        b = tab.encode_flp_json_content(recs, present, parts, NOW, MONO, names, AGENT, RECEIVED)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        a = tab.encode_pb_netev(recs, present, parts, rows, empty, NOW, MONO, AGENT, nf.intf_table(PB_NAMES))
        b = tab.encode_pb(recs, NOW, MONO, AGENT, nf.intf_table(PB_NAMES), present=present, parts={k: parts[k] for k in parts})
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        rows[:, 1] = 3                                                                # a row beyond the table counts as none
        c = tab.encode_flp_json_netev(recs, present, parts, rows, empty, NOW, MONO, names, AGENT, RECEIVED)
        assert c[0].tobytes() == j[0].tobytes()


def test_table_of_another_handle_is_refused(nf, tab):
    with nf.NetevTable([]) as host_only:
        with pytest.raises(nf.NfaggError) as e:
            tab.netev_resolve(host_only, np.zeros(1, dtype=np.uint8), None, None)
        assert e.value.code == nf._lib.EINVAL


def test_map_tracer_with_a_python_decoder(nf, O, tab):
    """The MapTracer mirror over drained maps: JSON lines identical to the restatement, the decoder asked once per distinct
    cookie, and not again at the next eviction."""
    from test_map_merge import make_maps
    n_cpu = 4
    main_ids, main_vals, feats = make_maps(O, seed=11, n_pop=400, n_main=300, n_feat=250, n_cpu=n_cpu)
    for f in ("ssl_version", "tls_cipher_suite", "tls_key_share"):                     # one flow in five stays deferred
        main_vals[f][np.arange(len(main_vals)) % 5 != 0] = 0
    calls = []

    def decoder(cookie):
        calls.append(cookie)
        if cookie[0] % 4 == 0:
            raise ValueError("no such sample")
        if cookie[0] % 4 == 1:
            return b"event %d" % cookie[1]
        return ("drop" if cookie[0] % 4 == 2 else "allow", "NetpolNode", "n", "", "Ingress", b"acl %d" % (cookie[1] % 3))

    drained = (main_ids, main_vals, feats, n_cpu)
    mt = nf.MapTracer(nf.GPUMapFetcher(tab, lambda: drained), 0, 0, sample_decoder=decoder, clock=lambda: NOW, mono_clock=lambda: MONO)
    got = mt.evictFlowsJSON(G.table(nf, NAMES), AGENT, RECEIVED)
    recs, present, parts, _ = tab.map_merge(main_ids, main_vals, feats, n_cpu)
    ref_calls = []

    def ref_decoder(c):
        ref_calls.append(c)
        try:
            return decoder(c)
        except ValueError:
            return None

    (wp, wd, wrows, events, _), answers, n_calls = N.resolve_loop(present, parts["network_events"], parts["drops"], ref_decoder)
    dparts = dict(parts, drops=wd.copy().view(nf.PKT_DROP).reshape(-1))
    G.check(got, N.encode_json(recs, wp, dparts, events, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED))
    distinct = {bytes(c) for i in range(len(recs)) if present[i] & N.FEAT_NETEV
                for k, c in enumerate(parts["network_events"]["network_events"][i]) if parts["network_events"]["packets"][i][k]}
    assert mt.decoderCalls == len(distinct) == n_calls and len(distinct) > 3
    again = mt.evictFlowsJSON(G.table(nf, NAMES), AGENT, RECEIVED)
    assert mt.decoderCalls == len(distinct) and again[0].tobytes() == got[0].tobytes()
