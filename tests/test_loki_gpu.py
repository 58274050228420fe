"""write loki on the device (nfagg_loki_plan / nfagg_loki_write; csrc/nfagg_loki.hip) through the C ABI, host and device entry
points. Every batch's PushRequest body is compared byte for byte with the restatement of tests/loki_ref.py over the maps of
tests/flp_json_net_ref.py, and independently decoded with google.protobuf (tests/test_loki_cpu.py) and compared as a set of
(labels, ordered entries). Shapes are the smallest at which a path can go wrong.

Not reachable on the device, and therefore pinned on the restatement alone (test_loki_cpu.py): an entry below 128 bytes (the
shortest line, a non-IP flow with an empty interface name, has 191); a time outside [year 1, year 10000), which no int64
nanosecond count reaches — the product leaving int64 is the deferral that occurs."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_k8s_ref as K  # noqa: E402
import flp_json_tls_ref as RT  # noqa: E402
import loki_ref as LR  # noqa: E402
import netev_ref as N  # noqa: E402
import test_conntrack_gpu as CG  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_flp_json_k8s_gpu as KG  # noqa: E402
import test_flp_json_net_cpu as NC  # noqa: E402
import test_flp_json_net_gpu as NG  # noqa: E402
import test_flp_json_tls_gpu as TG  # noqa: E402
import test_netev_gpu as E  # noqa: E402
from test_loki_cpu import OPERATOR, decode_push_request  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, NOW, MONO, RECEIVED, REPORTER, LAYER = G.NAMES, G.NOW, G.MONO, G.RECEIVED, NG.REPORTER, KG.LAYER
RULES = dict(direction=True, labels=NG.CATEGORIES, flags=True)
LOKI_NOW = 1_700_000_009_000_000_042
BASE = dict(timestampLabel="TimeFlowEndMs", timestampScale="1ms")
ALL_KEYS = ["%sK8S_%s" % (side, f) for side in ("Src", "Dst") for f in ("Namespace", "Name", "Type", "OwnerName", "OwnerType", "NetworkName", "HostIP", "HostName", "Zone")] + \
           ["SrcSubnetLabel", "DstSubnetLabel", "FlowDirection", "K8S_FlowLayer", "_RecordType"]


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


@pytest.fixture(scope="module")
def go_names(nf, tab):
    with tab.tls_names() as t:
        yield t, RT.table_of(nf.GO_TLS_NAMES)


def device_call(nf, tab, tls, k8s, net, lt, recs, ids, names, now, mono, received, loki_now, texts_of, present=None, parts=None, rows=None, ne_table=None):
    """nfagg_loki_plan_device and nfagg_loki_write_device on device pointers: canaries behind every output, the size query, a buffer
    one byte short (NFAGG_TRUNCATED, nothing written), then the write."""
    import torch
    L = nf._lib
    n = len(recs)
    d_recs, d_ids = (E.dev(recs) if n else None), (E.dev(np.ascontiguousarray(ids, dtype=np.uint64)) if ids is not None and n else None)
    o, keep = nf.flp_options(now, mono, names, REPORTER, received, b"unknown")
    cap_s, cap_g = max(n, 1), max(n, 1)
    d_streams = torch.full((cap_s * 20 + 24,), 0xAB, dtype=torch.uint8, device="cuda")
    d_groups = torch.full((cap_g * 24 + 24,), 0xAB, dtype=torch.uint8, device="cuda")
    d_def = torch.full((n + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    counts = L.LokiCounts()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    feat = d_rows = None
    if present is not None and n:
        d_present = E.dev(present)
        d_parts = {k: E.dev(v) for k, v in parts.items() if k != "network_events"}
        feat, _ = tab._pb_features(n, d_present.data_ptr(), {k: v.data_ptr() for k, v in d_parts.items()}, device=True)
        d_rows = E.dev(rows) if rows is not None else None
    f_args = (C.byref(feat) if feat is not None else None, ptr(d_rows), ne_table._t if d_rows is not None else None)
    rc = L.lib.nfagg_loki_plan_device(tab._h, ptr(d_recs), n, *f_args, tls._t, k8s._t, net._t, ptr(d_ids), C.byref(o), lt._t, loki_now, ptr(d_streams), cap_s,
                                      ptr(d_groups), cap_g, ptr(d_def), C.byref(counts))
    assert rc == L.OK, nf._lib.lib.nfagg_last_error(tab._h)
    torch.cuda.synchronize()
    s_raw, g_raw, deferred = d_streams.cpu().numpy(), d_groups.cpu().numpy(), d_def.cpu().numpy()
    assert (s_raw[counts.n_streams * 20:] == 0xAB).all() and (g_raw[counts.n_groups * 24:] == 0xAB).all() and (deferred[n:] == 0xAB).all()
    streams = s_raw[:counts.n_streams * 20].view(nf.LOKI_STREAM)
    groups = g_raw[:counts.n_groups * 24].view(nf.LOKI_GROUP)
    texts = texts_of(streams)
    blob = b"".join(texts)
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(t) for t in texts], dtype=np.uint64)
    nb = counts.n_batches
    d_boff = torch.full((nb + 1 + 4,), -1, dtype=torch.int64, device="cuda")
    d_bent = torch.full((nb + 4,), -1, dtype=torch.int32, device="cuda")
    need = C.c_size_t(0)
    w_args = (tab._h, blob, off.ctypes.data_as(C.c_void_p))
    rc = L.lib.nfagg_loki_write_device(*w_args, None, 0, ptr(d_boff), ptr(d_bent), C.byref(need))
    assert rc == (L.TRUNCATED if need.value else L.OK)
    total = need.value
    d_out = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    if total:
        rc = L.lib.nfagg_loki_write_device(*w_args, ptr(d_out), total - 1, ptr(d_boff), ptr(d_bent), C.byref(need))
        torch.cuda.synchronize()
        assert rc == L.TRUNCATED and need.value == total and bool((d_out == 0xAB).all())
    rc = L.lib.nfagg_loki_write_device(*w_args, ptr(d_out), total, ptr(d_boff), ptr(d_bent), C.byref(need))
    torch.cuda.synchronize()
    out, boff, bent = d_out.cpu().numpy(), d_boff.cpu().numpy(), d_bent.cpu().numpy()
    assert rc == L.OK and need.value == total and (out[total:] == 0xAB).all() and (boff[nb + 1:] == -1).all() and (bent[nb:] == -1).all()
    assert int(boff[nb]) == total
    return streams, groups, deferred[:n], counts, out[:total].tobytes(), boff[:nb + 1], bent[:nb]


def run(nf, tab, go_names, entries, recs, config, ids=None, layer=LAYER, rules=RULES, now=NOW, mono=MONO, received=RECEIVED, loki_now=LOKI_NOW, texts=None,
        device=True, present=None, parts=None, answers=None, ne_table=None):
    """Both entry points against the restatement. texts(streams) -> label texts overrides the product's rendering. Returns the
    restatement's (bodies, batches, deferred) and the host call's streams and groups."""
    tls, tls_ref = go_names
    w = nf.WriteLoki(dict(BASE, **config))
    names = G.table(nf, NAMES)
    rp, rparts, events, rows = present, parts, None, None
    if answers is not None:                                  # the sample decoder's answers: resolved by the restatement, and on the device below
        res = N.resolve(present, parts["network_events"], parts["drops"], answers)
        rp, rparts, events = res[0], dict(parts, drops=res[1]), res[3]
        present, d_out, rows, missing, _ = tab.netev_resolve(ne_table, present, parts["network_events"], parts["drops"])
        assert set(missing) == res[4] and rows.tolist() == res[2].tolist()
        parts = dict(parts, drops=d_out)
    maps = LR.flow_maps(recs, tls_ref, K.table_of(entries), layer, rules, now, mono, G.rows(NAMES), REPORTER, received, ids, rp, rparts, events)
    want_bodies, want_batches, want_def = LR.write_loki(maps, w.sane_labels, w.ignore_list, w.static_labels, w.timestamp_label, w.timestamp_scale, w.batch_size, loki_now)
    call_now = w.now_of_call(loki_now, received)
    with tab.k8s_table(entries, layer) as k8s, NC.net_table(nf, rules, tab) as net, tab.loki_table(w, k8s, net) as lt:
        texts_of = texts or lt.labels_of
        feats = dict(present=present, parts=parts, rows=rows, netev_table=ne_table if rows is not None else None)
        rc, streams, groups, deferred, counts = tab.loki_plan(recs, tls, k8s, net, lt, now, mono, names, REPORTER, received, b"unknown", ids, call_now, **feats)
        assert rc == nf.OK
        rc, buf, boffs, bents = tab.loki_write(texts_of(streams), counts.n_batches)
        assert rc == nf.OK
        got = [(streams, groups, deferred, counts, np.asarray(buf).tobytes(), boffs, bents)]
        if device:
            got.append(device_call(nf, tab, tls, k8s, net, lt, recs, ids, names, now, mono, received, call_now, texts_of, present, parts, rows, ne_table))
    for streams, groups, deferred, counts, body, boffs, bents in got:
        assert np.flatnonzero(deferred).tolist() == want_def and counts.n_deferred == len(want_def)
        assert counts.n_batches == len(want_bodies) and len(boffs) == len(want_bodies) + 1
        bodies = [body[int(boffs[b]):int(boffs[b + 1])] for b in range(counts.n_batches)]
        for b, (g, wb) in enumerate(zip(bodies, want_bodies)):
            if g != wb:
                k = next((i for i, (x, y) in enumerate(zip(g, wb)) if x != y), min(len(g), len(wb)))
                raise AssertionError("batch %d differs at byte %d of %d / %d:\n got %r\nwant %r" % (b, k, len(g), len(wb), g[max(0, k - 60):k + 60], wb[max(0, k - 60):k + 60]))
            assert sorted(decode_push_request(g)) == sorted((t, e) for t, e in want_batches[b])      # the independent decode, as a set of streams
        assert len(body) == sum(len(x) for x in want_bodies)
        assert bents.tolist() == [sum(len(e) for _, e in b) for b in want_batches]
        assert counts.n_groups == sum(len(b) for b in want_batches) == len(groups)
        assert [(int(g["batch"]), int(g["n_entries"])) for g in groups] == [(b, len(e)) for b, wb in enumerate(want_batches) for _, e in wb]
        first = [int(s["first_flow"]) for s in streams]
        assert first == sorted(first) and len(set(first)) == len(first)
    return (want_bodies, want_batches, want_def), got[0][0], got[0][1]


def same_flows(nf, n, src="10.0.0.5", dst="10.0.2.200"):
    return NG.ip_records(nf, [(src, dst)] * n)


def line_len(batches):
    return len(batches[0][0][1][0][2])


ENTRIES = [("10.0.0.5", dict(KG.INFOS[0], name="a")), ("10.0.2.200", dict(KG.INFOS[4], name="b"))]


# ---- record counts, conntrack on and off
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
@pytest.mark.parametrize("conn", [False, True])
def test_record_counts_with_and_without_hash_ids(nf, O, tab, go_names, n, conn):
    """The seeded stream: untracked flows between tracked ones, sides without a row, empty namespaces, an owner name that is empty
    but present, one that is not valid UTF-8 (KG.INFOS); several batches."""
    recs = CG.seeded(nf, O, n, 5 + n)
    ids = tab.conn_fold(recs, NOW, MONO, cap=4096)[3] if conn else None
    (bodies, batches, deferred), streams, _ = run(nf, tab, go_names, KG.entries_for(recs), recs, dict(labels=OPERATOR, batchSize=4000, staticLabels={"app": "flows"}), ids)
    if n >= 63:
        assert len(bodies) > 3 and len(streams) > 3 and not deferred
        assert conn == any(b'_RecordType="flowLog"' in t for b in batches for t, _ in b)
        assert all(b"_RecordType" not in e[2] for b in batches for _, es in b for e in es) and conn == any(b'"_HashId":"' in e[2] for b in batches for _, es in b for e in es)


@pytest.fixture(scope="module")
def netev_table(tab):
    with tab.netev_table(E.ANSWERS.items()) as t:
        yield t


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("conn", [False, True])
@pytest.mark.parametrize("policy", [0, 1, 2])
def test_all_three_policies_with_and_without_hash_ids(nf, O, tab, go_names, netev_table, policy, conn, n):
    """The plain line, full flow contents (DNS, drops, xlat, RTT / IPsec, QUIC parts) and contents with network events, under the
    operator's label set and with every other maskable key ignored in turn with it; several batches."""
    recs, present, parts, answers = TG.policy_inputs(nf, O, n, 40 + n, policy)
    ids = tab.conn_fold(recs, NOW, MONO, cap=4096)[3] if conn else None
    entries = KG.entries_for(recs)
    for cfg in (dict(labels=OPERATOR, batchSize=6000, staticLabels={"app": "flows"}), dict(labels=OPERATOR, ignoreList=[k for k in ALL_KEYS if k not in OPERATOR] + ["_HashId"], batchSize=1 << 20)):
        (bodies, batches, deferred), streams, _ = run(nf, tab, go_names, entries, recs, cfg, ids, present=present, parts=parts, answers=answers, ne_table=netev_table)
        lines = b"".join(e[2] for b in batches for _, es in b for e in es)
        if n >= 65:
            assert not deferred and len(streams) > 3 and (policy == 0) == (b'"DnsId":' not in lines) and (policy == 2) == (b'"NetworkEvents":[' in lines)


def test_feature_argument_checks(nf, O, tab, go_names, netev_table):
    L = nf._lib
    recs, present, parts, _ = TG.policy_inputs(nf, O, 4, 3, 1)
    w = nf.WriteLoki(BASE)
    with tab.k8s_table([], None) as k8s, NC.net_table(nf, RULES, tab) as net, tab.loki_table(w, k8s, net) as lt:
        o, keep = nf.flp_options(NOW, MONO, G.table(nf, NAMES), REPORTER, RECEIVED, b"unknown")
        counts = L.LokiCounts()
        rows = np.zeros((4, 4), dtype=np.uint16)
        args = (go_names[0]._t, k8s._t, net._t, None, C.byref(o), lt._t, 0, None, 0, None, 0, None, C.byref(counts))
        bad = L.PbFeatures(struct_size=8)
        for f_args, text in (((C.byref(bad), None, None), b"struct_size"), ((None, rows.ctypes.data_as(C.c_void_p), None), b"rows and table go together"),
                             ((None, rows.ctypes.data_as(C.c_void_p), netev_table._t), b"without the flows' feature parts")):
            assert L.lib.nfagg_loki_plan(tab._h, recs.ctypes.data_as(C.c_void_p), 4, *f_args, *args) == L.EINVAL and text in L.lib.nfagg_last_error(tab._h)
    assert [L.lib.nfagg_loki_max_entry(p) for p in range(4)] == [L.lib.nfagg_flp_json_conn_max_line(p) - 1 + 27 for p in range(3)] + [0]


# ---- wave and stream shapes
def many_sources(nf, k, n, order):
    srcs = ["10.9.%d.%d" % (i // 250, 1 + i % 250) for i in range(k)]
    entries = [(s, dict(namespace="ns-%d" % i, name="p", kind="Pod")) for i, s in enumerate(srcs)]
    return NG.ip_records(nf, [(srcs[order(j)], "10.0.2.200") for j in range(n)]), entries


def test_sixty_four_flows_of_one_wave_in_sixty_four_streams(nf, tab, go_names):
    recs, entries = many_sources(nf, 64, 64, lambda j: (j * 37) % 64)
    (_, batches, _), streams, groups = run(nf, tab, go_names, entries, recs, dict(labels=["SrcK8S_Namespace"], batchSize=1 << 20))
    assert len(streams) == 64 and len(batches) == 1 and len(batches[0]) == 64 and [int(s["first_flow"]) for s in streams] == list(range(64))


def test_two_streams_interleaved_flow_by_flow(nf, tab, go_names):
    recs, entries = many_sources(nf, 2, 131, lambda j: j % 2)
    (_, batches, _), streams, groups = run(nf, tab, go_names, entries, recs, dict(labels=["SrcK8S_Namespace"], batchSize=1 << 20))
    assert len(streams) == 2 and [len(e) for _, e in batches[0]] == [66, 65]


def test_a_group_begins_on_a_waves_last_lane(nf, tab, go_names):
    recs, entries = many_sources(nf, 2, 70, lambda j: 0 if j < 63 else 1)
    (_, batches, _), streams, groups = run(nf, tab, go_names, entries, recs, dict(labels=["SrcK8S_Namespace"], batchSize=1 << 20))
    assert [len(e) for _, e in batches[0]] == [63, 7]                                          # the second group's header and first entry: position 63


def test_one_stream_spans_three_batches_and_the_cut_is_strictly_greater(nf, tab, go_names):
    recs = same_flows(nf, 30)
    (_, batches, _), _, _ = run(nf, tab, go_names, ENTRIES, recs, dict(labels=OPERATOR, batchSize=1 << 20))
    ll = line_len(batches)
    for size, want in ((10 * ll, [10, 10, 10]), (10 * ll - 1, [9, 9, 9, 3]), (1, [1] * 30), (30 * ll, [30]), (30 * ll - 1, [29, 1])):
        (_, batches, _), streams, groups = run(nf, tab, go_names, ENTRIES, recs, dict(labels=OPERATOR, batchSize=size))
        assert [sum(len(e) for _, e in b) for b in batches] == want and len(streams) == 1 and len(groups) == len(want)


# ---- varint edges
def test_a_stream_whose_size_straddles_2_to_the_14_and_2_to_the_21(nf, tab, go_names):
    (bodies, batches, _), _, _ = run(nf, tab, go_names, ENTRIES, same_flows(nf, 2), dict(labels=OPERATOR, batchSize=10 << 20))
    one = len(LR.marshal_stream(b"", batches[0][0][1][:1]))                                   # one framed entry
    head = len(LR.marshal_stream(batches[0][0][0], []))
    for edge in (1 << 14, 1 << 21):
        k = (edge - head) // one                                                              # k entries stay below the edge, k + 1 reach it
        for n in (k, k + 1):
            (bodies, batches, _), _, groups = run(nf, tab, go_names, ENTRIES, same_flows(nf, n), dict(labels=OPERATOR, batchSize=10 << 20))
            size = head + int(groups[0]["entry_bytes"])
            assert len(bodies) == 1 and (size < edge) == (n == k) and len(bodies[0]) == 1 + len(LR.varint(size)) + size


@pytest.mark.parametrize("size", [2, 127, 128, 4096])
def test_label_text_sizes(nf, tab, go_names, size):
    text = b"{}" if size == 2 else b'{a="' + b"x" * (size - 6) + b'"}'
    assert len(text) == size
    (bodies, batches, _), _, _ = run(nf, tab, go_names, ENTRIES, same_flows(nf, 3), dict(batchSize=1 << 20, staticLabels={} if size == 2 else {"a": "x" * (size - 6)}),
                                     texts=lambda streams: [text] * len(streams))
    assert batches[0][0][0] == text and len(bodies) == 1


def test_label_text_outside_its_bounds_is_refused(nf, tab, go_names):
    w = nf.WriteLoki(BASE)
    with tab.k8s_table(ENTRIES, LAYER) as k8s, NC.net_table(nf, RULES, tab) as net, tab.loki_table(w, k8s, net) as lt:
        rc, streams, groups, deferred, counts = tab.loki_plan(same_flows(nf, 3), go_names[0], k8s, net, lt, NOW, MONO, G.table(nf, NAMES), REPORTER, RECEIVED)
        for text in (b"{", b"{" + b"x" * 4095 + b"}"):
            with pytest.raises(nf.NfaggError) as e:
                tab.loki_write([text], counts.n_batches)
            assert e.value.code == nf._lib.EINVAL and "not 2 .. 4096" in str(e.value)


# ---- timestamps: with now = mono = 0 a flow's TimeFlowEndMs is its end / 1e6
def timed(nf, ms_values):
    recs = same_flows(nf, len(ms_values))
    recs["metrics"]["end_mono_time_ts"] = np.array([(ms * 10 ** 6) % (1 << 64) for ms in ms_values], dtype=np.uint64)
    return recs


def test_timestamp_shapes(nf, tab, go_names):
    """0: now; a multiple of 1000: no nanos field; below 1000: no seconds field; negative: a ten-byte varint and a normalised
    remainder; products of ms * 1e6 = ms * 15625 * 64 beyond 2^53: rounding, with ties (ms * 15625 = 2 mod 4) going to even."""
    ms = [0, 5000, 999, 1, -1, -1500, -2000, 1760000000000, 1760000000001, 1760000000002, 1760000000003, 1760000000005, 1760000000006, 1760000000007, 9007199255]
    recs = timed(nf, ms)
    (bodies, batches, deferred), _, _ = run(nf, tab, go_names, ENTRIES, recs, dict(batchSize=1 << 20), now=0, mono=0)
    stamps = [(e[0], e[1]) for e in batches[0][0][1]]
    assert not deferred and stamps[0] == (LOKI_NOW // 10 ** 9, LOKI_NOW % 10 ** 9) and stamps[1] == (5, 0) and stamps[2] == (0, 999000000) and stamps[4] == (-1, 999000000)
    assert stamps[5] == (-2, 500000000) and stamps[6] == (-2, 0)
    assert stamps[8] != (1760000000, 1000000) and stamps[9] in ((1760000000, 1999872), (1760000000, 2000128))        # rounded; the tie went to an even mantissa


def test_timestamp_scale_of_a_second_and_the_int64_edge(nf, tab, go_names):
    """ms * 1e9: 9223372036 stays inside int64, 9223372037 leaves it and is deferred; the batches around it are those of the other flows."""
    ms = [1000, 9223372036, 9223372037, 1760000000000, 2000, -9223372037, -9223372036, 3000]
    (bodies, batches, deferred), _, _ = run(nf, tab, go_names, ENTRIES, timed(nf, ms), dict(batchSize=1, timestampScale="1s"), now=0, mono=0)
    assert deferred == [2, 3, 5] and len(bodies) == 5
    (b2, _, d2), _, _ = run(nf, tab, go_names, ENTRIES, timed(nf, [m for i, m in enumerate(ms) if i not in deferred]), dict(batchSize=1, timestampScale="1s"), now=0, mono=0)
    assert b2 == bodies and not d2


def test_time_received_as_the_timestamp_and_the_start_time(nf, O, tab, go_names):
    recs = same_flows(nf, 5)
    (_, batches, _), _, _ = run(nf, tab, go_names, ENTRIES, recs, dict(timestampLabel="TimeReceived", timestampScale="1s", batchSize=1 << 20))
    assert all(e[:2] == (RECEIVED, 0) for e in batches[0][0][1])
    (_, batches, _), _, _ = run(nf, tab, go_names, ENTRIES, recs, dict(timestampLabel="TimeReceived", timestampScale="1s", batchSize=1 << 20), received=0)
    assert all(e[:2] == (LOKI_NOW // 10 ** 9, 42) for e in batches[0][0][1])                  # 0: timeNow()
    run(nf, tab, go_names, ENTRIES, CG.seeded(nf, O, 65, 9), dict(timestampLabel="TimeFlowStartMs", batchSize=3000))


# ---- masking and presence
@pytest.mark.parametrize("how", ["labels", "ignoreList"])
def test_every_maskable_key_alone_and_all_together(nf, O, tab, go_names, how):
    recs = CG.seeded(nf, O, 65, 70)
    ids = tab.conn_fold(recs, NOW, MONO, cap=4096)[3]
    entries = KG.entries_for(recs)
    seen = set()
    for keys in [[k] for k in ALL_KEYS] + [ALL_KEYS] + ([["_HashId"], ALL_KEYS + ["_HashId"]] if how == "ignoreList" else []):
        (bodies, batches, _), streams, _ = run(nf, tab, go_names, entries, recs, {how: keys, "batchSize": 20000}, ids)
        lines = b"".join(e[2] for b in batches for _, es in b for e in es)
        for k in keys:
            assert b'"%s":' % k.encode() not in lines
        seen.add(len(streams))
    assert max(seen) > 3 if how == "labels" else seen == {1}
    if how == "labels":
        with pytest.raises(ValueError):
            nf.WriteLoki(dict(BASE, labels=["_HashId"]))


def test_presence_rules_of_the_label_fields(nf, tab, go_names):
    """No row; an empty namespace (absent); an empty owner name (present, a value); an owner name that is not valid UTF-8 (gone from
    the labels and from the line); a subnet label that is empty, and two categories with one name."""
    infos = [dict(namespace="shop", name="a", kind="Pod", owner_name="cart"), dict(namespace="", name="b", kind="Pod", owner_name=""),
             dict(namespace="shop", name="c", kind="Pod", owner_name=b"bad\xff"), dict(namespace="shop", name="d", kind="Pod", owner_name="cart")]
    entries = [("10.0.0.%d" % (k + 1), info) for k, info in enumerate(infos)]
    rules = dict(direction=True, flags=False, labels=[("lan", ["10.0.0.0/30"]), ("", ["10.0.0.4/32"]), ("lan", ["10.0.0.5/32"]), ("wan", ["0.0.0.0/0"])])
    recs = NG.ip_records(nf, [("10.0.0.%d" % s, "10.0.0.%d" % d) for s in range(1, 8) for d in (1, 2, 5, 7)])
    cfg = dict(labels=["SrcK8S_Namespace", "SrcK8S_OwnerName", "DstK8S_OwnerName", "SrcSubnetLabel", "DstSubnetLabel"], batchSize=5000)
    (bodies, batches, _), streams, _ = run(nf, tab, go_names, entries, recs, cfg, rules=rules)
    texts = {t for b in batches for t, _ in b}
    assert b'{DstK8S_OwnerName="cart", DstSubnetLabel="lan", SrcK8S_OwnerName="", SrcSubnetLabel="lan"}' in texts          # row b: no namespace label, owner ""
    assert b'{DstK8S_OwnerName="cart", DstSubnetLabel="lan", SrcK8S_Namespace="shop", SrcSubnetLabel="lan"}' in texts      # row c: the owner name is gone
    assert not any(b"bad" in t for t in texts) and not any(b'"SrcK8S_OwnerName":"bad' in e[2] for b in batches for _, es in b for e in es)
    # 10.0.0.4 (row d): the empty category ends the search, no SrcSubnetLabel; 10.0.0.6 has no row and falls through to "wan"
    assert b'{DstK8S_OwnerName="cart", DstSubnetLabel="lan", SrcK8S_Namespace="shop", SrcK8S_OwnerName="cart"}' in texts
    assert b'{DstK8S_OwnerName="cart", DstSubnetLabel="lan", SrcSubnetLabel="wan"}' in texts
    # rows a and d, and the two "lan" categories, share their streams
    assert len(streams) == len(texts)


# ---- errors
def test_truncated_on_both_caps_and_write_without_a_plan(nf, tab, go_names):
    L = nf._lib
    recs, entries = many_sources(nf, 8, 40, lambda j: j % 8)
    w = nf.WriteLoki(dict(BASE, labels=["SrcK8S_Namespace"], batchSize=2000))
    with nf.FlowTable(max_entries=64) as fresh:
        with pytest.raises(nf.NfaggError) as e:
            fresh.loki_write([b"{}"], 1)
        assert e.value.code == L.EINVAL and "no plan" in str(e.value)
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, RULES, tab) as net, tab.loki_table(w, k8s, net) as lt:
        args = (recs, go_names[0], k8s, net, lt, NOW, MONO, G.table(nf, NAMES), REPORTER, RECEIVED)
        rc, streams, groups, deferred, counts = tab.loki_plan(*args)
        assert rc == nf.OK and counts.n_streams == 8 and counts.n_groups > 8
        for sc, gc in ((7, 4096), (8, counts.n_groups - 1), (0, 0)):
            o, keep = nf.flp_options(NOW, MONO, G.table(nf, NAMES), REPORTER, RECEIVED, b"unknown")
            s, g = np.full(max(sc, 1) * 20, 0xAB, dtype=np.uint8), np.full(max(gc, 1) * 24, 0xAB, dtype=np.uint8)
            c = L.LokiCounts()
            rc = L.lib.nfagg_loki_plan(tab._h, recs.ctypes.data_as(C.c_void_p), len(recs), None, None, None, go_names[0]._t, k8s._t, net._t, None, C.byref(o), lt._t, LOKI_NOW,
                                       s.ctypes.data_as(C.c_void_p) if sc else None, sc, g.ctypes.data_as(C.c_void_p) if gc else None, gc, None, C.byref(c))
            assert rc == L.TRUNCATED and (c.n_streams, c.n_groups, c.n_batches) == (8, counts.n_groups, counts.n_batches)
            assert (s == 0xAB).all() and (g == 0xAB).all()                                       # nothing written
            with pytest.raises(nf.NfaggError) as e:
                tab.loki_write([b"{}"] * 8, counts.n_batches)
            assert "no plan" in str(e.value)
        with nf.LokiTable(w, nf.K8sTable(entries, LAYER, None), nf.NetTable(0, (), None)) as host_only:
            with pytest.raises(nf.NfaggError) as e:
                tab.loki_plan(recs, go_names[0], k8s, net, host_only, NOW, MONO, G.table(nf, NAMES), REPORTER, RECEIVED)
            assert "was not created for this handle" in str(e.value)


# ---- the writer behind a filter, end to end
def test_loki_writer_behind_a_filter(nf, O, tab, go_names):
    recs = CG.seeded(nf, O, 200, 31)
    entries = KG.entries_for(recs)
    cfg = dict(BASE, labels=OPERATOR, batchSize=6000, staticLabels={"app": "netobserv-flowcollector"})
    w = nf.WriteLoki(cfg)
    sent = []
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, RULES, tab) as net:
        spec = nf.TransformFilter(dict(rules=[dict(type="keep_entry_query", keepEntryQuery="Proto = 6 or Proto = 17", keepEntrySampling=0)]), k8s_entries=entries,
                                  labels=net.labels, layer=True, net_flags=net.flags)
        with tab.filter(spec, k8s, net) as flt:
            writer = nf.LokiWriter(tab, w, go_names[0], k8s, net, names=G.table(nf, NAMES), agent_ip=REPORTER, conntrack=True, send=sent.append)
            exp = nf.DirectFLPJSON(tab, io.BytesIO(), G.table(nf, NAMES), REPORTER, time_received=lambda: RECEIVED, tls_names=go_names[0], k8s=k8s, net=net,
                                   filter=nf.StageFilter(flt, seed=1), loki=writer)
            kept = np.isin(recs["metrics"]["eth_protocol"], (0x0800, 0x86DD)) & np.isin(recs["id"]["transport_protocol"], (6, 17))
            assert exp.ExportEvicted(recs, NOW, MONO) == int(kept.sum()) > 20
            writer.loki.close()
    sub = recs[kept]
    ids = tab.conn_fold(sub, NOW, MONO, cap=4096)[3]
    maps = LR.flow_maps(sub, go_names[1], K.table_of(entries), LAYER, RULES, NOW, MONO, G.rows(NAMES), REPORTER, RECEIVED, ids)
    want, _, want_def = LR.write_loki(maps, w.sane_labels, w.ignore_list, w.static_labels, w.timestamp_label, w.timestamp_scale, w.batch_size, NOW)
    assert sent == want == exp.loki_bodies and exp.loki_deferred == want_def == [] and len(want) > 2 and writer.batches == len(want)
    with pytest.raises(ValueError):
        nf.DirectFLPJSON(tab, io.BytesIO(), loki=writer)


def test_map_tracer_with_loki(nf, O, tab, go_names):
    """MapTracer.evictFlowsJSON(loki=): the merged flows with their parts and the sample decoder's events end in PushRequest bodies."""
    from test_map_merge import make_maps
    n_cpu = 4
    main_ids, main_vals, feats = make_maps(O, seed=11, n_pop=400, n_main=300, n_feat=250, n_cpu=n_cpu)
    main_vals["eth_protocol"] = 0x86DD
    decoder = lambda cookie: None if cookie[0] % 2 == 0 else b"event %d" % cookie[1]  # noqa: E731
    mrecs, present, parts, _ = tab.map_merge(main_ids, main_vals, feats, n_cpu)
    entries = KG.entries_for(mrecs)
    (wp, wd, wrows, events, _), answers, _ = N.resolve_loop(present, parts["network_events"], parts["drops"], decoder)
    w = nf.WriteLoki(dict(BASE, labels=OPERATOR, batchSize=20000))
    maps = LR.flow_maps(mrecs, go_names[1], K.table_of(entries), LAYER, RULES, NOW, MONO, G.rows(NAMES), REPORTER, RECEIVED, None, wp, dict(parts, drops=wd), events)
    want, _, want_def = LR.write_loki(maps, w.sane_labels, w.ignore_list, w.static_labels, w.timestamp_label, w.timestamp_scale, w.batch_size, NOW)
    mt = nf.MapTracer(nf.GPUMapFetcher(tab, lambda: (main_ids, main_vals, feats, n_cpu)), 0, 0, sample_decoder=decoder, clock=lambda: NOW, mono_clock=lambda: MONO)
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, RULES, tab) as net:
        writer = nf.LokiWriter(tab, w, go_names[0], k8s, net, names=G.table(nf, NAMES), agent_ip=REPORTER)
        bodies, late, held = mt.evictFlowsJSON(G.table(nf, NAMES), REPORTER, RECEIVED, tls_names=go_names[0], k8s=k8s, net=net, loki=writer)
        writer.loki.close()
    assert bodies == want and late == want_def and held == [] and len(want) > 2 and any(events) and any(b'"NetworkEvents":[' in b for b in want)
    with pytest.raises(ValueError):
        mt.evictFlowsJSON(loki=writer)
