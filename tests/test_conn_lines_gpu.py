"""extract conntrack's flow logs as direct-FLP JSON lines on the GPU (nfagg_encode_flp_json_conn; csrc/nfagg_conn_meta.h) through
the C ABI, host and device entry points, all three policies. Expected, per flow: nothing for a flow the stage does not track; the
line of the restatement of tests/flp_json_net_ref.py with ,"_HashId":"<hex>","_RecordType":"flowLog" spliced in front of its
closing brace for every other. Whether a flow is tracked is decided here from the record (an IP ethertype and protocol 6, 17 or
132), the hex text by Python's "%x". Records, namer table, parts, network events, informer answers and rules are those of the
transform network tests; the seeded stream and its ids are those of test_conntrack_gpu.py.

The second half of the file has the conversation records (nfagg_encode_conn_json; csrc/nfagg_conn_json.hip): every byte, offset and
deferred flag against tests/conn_json_ref.py on the conversations of tests/conn_cases.py.

The end of the file has conntrack.ConnTrack.extract_lines: the stage's whole output for four calls, byte for byte against the record
stream of tests/conntrack_ref.py's Extract, each record marshalled and enriched by the restatements above."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conntrack_ref as CT  # noqa: E402
from conn_lines_ref import splice, tracked  # noqa: E402
import flp_json_k8s_ref as K  # noqa: E402
import flp_json_net_ref as R  # noqa: E402
import netev_ref as N  # noqa: E402
import test_conntrack_cpu as T  # noqa: E402
import test_conntrack_gpu as CG  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_flp_json_k8s_gpu as KG  # noqa: E402
import test_flp_json_net_cpu as NC  # noqa: E402
import test_flp_json_net_gpu as NG  # noqa: E402
import test_flp_json_tls_gpu as TG  # noqa: E402
import test_netev_gpu as E  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, NOW, MONO, RECEIVED, REPORTER = G.NAMES, G.NOW, G.MONO, G.RECEIVED, NG.REPORTER
LAYER, ALL, POLICIES = KG.LAYER, NG.ALL, (0, 1, 2)
ALL_WITH_LABELS = dict(ALL, labels=NG.CATEGORIES)
EDGE_IDS = [0, 1, 0xf, 0x10, (1 << 60) - 1, (1 << 64) - 1]


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


@pytest.fixture(scope="module")
def go_names(nf, tab):
    import flp_json_tls_ref as TR
    with tab.tls_names() as t:
        yield t, TR.table_of(nf.GO_TLS_NAMES)


@pytest.fixture(scope="module")
def netev_table(tab):
    with tab.netev_table(E.ANSWERS.items()) as t:
        yield t


def both_entry_points(nf, tab, tls, k8s, net, recs, ids, present, parts, ne_table, want_resolve, names=None, agent=REPORTER, received=RECEIVED, now=NOW,
                      mono=MONO):
    """The host call and the device call, with the protocol of test_flp_json_net_gpu.both_entry_points: the size query, a buffer
    one byte short (NFAGG_TRUNCATED, nothing written), then the write into a buffer with canaries behind it; the offsets have a
    canary behind them too."""
    import torch
    names = names if names is not None else G.table(nf, NAMES)
    n = len(recs)
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    rows = None
    if ne_table is not None:
        present, d_out, rows, missing, _ = tab.netev_resolve(ne_table, present, parts["network_events"], parts["drops"])
        assert set(missing) == want_resolve[4] and rows.tolist() == want_resolve[2].tolist()
        parts = dict(parts, drops=d_out)
    host = tab.encode_flp_json_conn(recs, tls, k8s, net, ids, now, mono, names, agent, received, present=present, parts=parts, rows=rows, netev_table=ne_table)
    d_recs = E.dev(recs) if n else None
    d_ids = E.dev(ids) if n else None
    d_present = E.dev(present) if present is not None and n else None
    d_parts = {k: E.dev(v) for k, v in (parts or {}).items() if k != "network_events"} if n else {}
    d_rows = E.dev(rows) if rows is not None and n else None
    kw = dict(d_present=d_present.data_ptr() if d_present is not None else 0, d_parts={k: v.data_ptr() for k, v in d_parts.items()},
              d_rows=d_rows.data_ptr() if d_rows is not None else 0, netev_table=ne_table if d_rows is not None else None)
    args = (d_recs.data_ptr() if n else 0, n, tls, k8s, net, d_ids.data_ptr() if n else 0, now, mono, names, agent, received)
    d_off = torch.full((n + 1 + 4,), -1, dtype=torch.int64, device="cuda")
    rc, need = tab.encode_flp_json_conn_device(*args, 0, 0, d_off.data_ptr(), **kw)
    assert rc == (nf.TRUNCATED if n else nf.OK) and need == len(host[0])               # the size query: the exact byte count
    d_out = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    if need:
        rc, short = tab.encode_flp_json_conn_device(*args, d_out.data_ptr(), need - 1, d_off.data_ptr(), **kw)
        torch.cuda.synchronize()
        assert rc == nf.TRUNCATED and short == need and bool((d_out == 0xAB).all())
    rc, wrote = tab.encode_flp_json_conn_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), **kw)
    torch.cuda.synchronize()
    out, off = d_out.cpu().numpy(), d_off.cpu().numpy()
    assert rc == nf.OK and wrote == need and (out[need:] == 0xAB).all() and (off[n + 1:] == -1).all()
    return host, (out[:need], off[:n + 1])


def run(nf, tab, tls, tls_ref, entries, layer, rules, recs, ids, present=None, parts=None, answers=None, ne_table=None, agent=REPORTER):
    events = res = None
    rp, rparts = present, parts
    if answers is not None:
        res = N.resolve(present, parts["network_events"], parts["drops"], answers)
        rp, rparts, events = res[0], dict(parts, drops=res[1]), res[3]
    net_want = R.encode(recs, tls_ref, K.table_of(entries), layer, rules, NOW, MONO, G.rows(NAMES), agent, RECEIVED, present=rp, parts=rparts, events=events)
    want = splice(net_want, recs, ids)
    with tab.k8s_table(entries, layer) as k8s, NC.net_table(nf, rules, tab) as net:
        for got in both_entry_points(nf, tab, tls, k8s, net, recs, ids, present, parts, ne_table if answers is not None else None, res, agent=agent):
            KG.check(got, want)
    return want


# ---- the seeded stream, its ids from the fold
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 513])
def test_the_seeded_stream_with_the_ids_of_the_fold(nf, O, tab, go_names, n):
    """The ids are nfagg_conn_fold's, checked against the restatement's before they are used: 0 for exactly the untracked flows."""
    recs = CG.seeded(nf, O, n, 5 + n)
    rc, parts, n_conns, ids, n_disc = tab.conn_fold(recs, T.NOW, T.MONO, cap=4096)
    assert rc == nf.OK and ids.tolist() == CT.fold(T.maps(recs, T.NOW, T.MONO), T.KD)[1]
    keep = tracked(recs)
    assert n_disc == int((~keep).sum()) and not ids[~keep].any()
    want = run(nf, tab, go_names[0], go_names[1], KG.entries_for(recs), LAYER, ALL_WITH_LABELS, recs, ids)
    assert len(want[1]) == n + 1 and want[0].count(b'"_RecordType":"flowLog"}\n') == int(keep.sum()) == want[0].count(b"\n")
    if n >= 513:
        assert 100 < keep.sum() < n - 100 and b'"SrcSubnetLabel"' in want[0] and b'"K8S_FlowLayer"' in want[0]


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("policy", POLICIES)
def test_each_policy_with_parts_and_network_events(nf, O, tab, go_names, netev_table, policy, n):
    recs, present, parts, answers = TG.policy_inputs(nf, O, 257, 61, policy)
    recs = recs.copy()
    recs["id"]["transport_protocol"][2::4] = 1                                    # untracked flows among flows that carry parts and events
    ids = np.random.default_rng(policy).integers(0, 1 << 64, 257, dtype=np.uint64)
    ids[:len(EDGE_IDS)] = EDGE_IDS
    ids[~tracked(recs)] = 0xDEAD                                                  # an untracked flow's id is not looked at
    cut = lambda a: a[:n] if a is not None else None  # noqa: E731
    want = run(nf, tab, go_names[0], go_names[1], KG.entries_for(recs), LAYER, ALL_WITH_LABELS, recs[:n], ids[:n], cut(present),
               {k: v[:n] for k, v in parts.items()} if parts else parts, answers, netev_table)
    assert b"dead" not in want[0] and want[0].count(b'"_HashId":"') == int(tracked(recs[:n]).sum())
    if n == 257 and policy:
        assert b'"DnsId"' in want[0] or b'"PktDrop' in want[0]
    if n == 257 and policy == 2:
        assert b'"NetworkEvents":[' in want[0]


# ---- crafted ids and lanes
def test_edge_ids_and_an_id_of_zero_on_a_tracked_flow(nf, tab, go_names):
    recs = NG.ip_records(nf, [("10.0.0.%d" % (k + 1), "2001:db8::%x" % (k + 1)) for k in range(len(EDGE_IDS))])
    recs["id"]["transport_protocol"] = [6, 17, 132, 6, 17, 132]
    want = run(nf, tab, go_names[0], go_names[1], [], None, R.RULES_OFF, recs, EDGE_IDS)[0].split(b"\n")
    tails = [b'"_HashId":"0"', b'"_HashId":"1"', b'"_HashId":"f"', b'"_HashId":"10"', b'"_HashId":"fffffffffffffff"', b'"_HashId":"ffffffffffffffff"']
    for line, tail in zip(want, tails):
        assert line.endswith(b"]," + tail + b',"_RecordType":"flowLog"}'), line          # behind Udns: the last key of a plain line


@pytest.mark.parametrize("name, untracked", [
    ("lane 0", [0]), ("lane 63", [63]), ("lanes 0 and 63 of two waves", [0, 63, 64, 127]), ("a whole wave", list(range(64, 128))),
    ("the first wave", list(range(64))), ("the last, partial wave", list(range(192, 200))), ("every flow", list(range(200))),
    ("all but the last flow", list(range(199))), ("all but the first flow", list(range(1, 200)))])
def test_untracked_flows_by_lane(nf, tab, go_names, name, untracked):
    """Four ways a flow is not tracked (ICMP, protocol 0, ARP, an ethertype of 0 with protocol 6), by lane of the write kernel's waves."""
    n = 200
    recs = NG.ip_records(nf, [("10.0.%d.%d" % (k % 4, k % 250 + 1), "10.0.2.%d" % (k % 100 + 1)) for k in range(n)], proto=17)
    for j, i in enumerate(untracked):
        if j % 4 == 0:
            recs["id"]["transport_protocol"][i] = 1
        elif j % 4 == 1:
            recs["id"]["transport_protocol"][i] = 0
        elif j % 4 == 2:
            recs["metrics"]["eth_protocol"][i] = 0x0806
        else:
            recs["metrics"]["eth_protocol"][i], recs["id"]["transport_protocol"][i] = 0, 6
    ids = np.arange(n, dtype=np.uint64) * 0x0123456789ABCDF + 1
    want = run(nf, tab, go_names[0], go_names[1], KG.entries_for(recs), LAYER, ALL_WITH_LABELS, recs, ids)
    lens = np.diff(want[1].astype(np.int64))
    assert sorted(np.flatnonzero(lens == 0).tolist()) == sorted(untracked) and want[0].count(b"\n") == n - len(untracked)


@pytest.mark.parametrize("policy", POLICIES)
def test_a_wave_spans_many_windows_and_every_line_is_the_longest(nf, tab, policy):
    """130 flows at the policy's worst case with sixteen hex digits: every line has exactly the bytes the write kernel sizes its
    window by. Every fifth flow is untracked, so the windows hold lines that are not neighbours in the batch."""
    n = 130
    case, line, ne_table = NG.worst_inputs(nf, tab, n, policy)
    lib = nf._lib.lib
    max_line = lib.nfagg_flp_json_conn_max_line(policy)
    assert max_line == lib.nfagg_flp_json_net_max_line(policy) + 53 == len(line) + 53
    window = (32768 - (16 if policy == 0 else 2048) - (max_line + 15) // 16 * 16) // 16 * 16      # FlpConnMeta<Base>::kWindow
    assert window >= 16384 and 51 * max_line > 2 * window                                          # a full wave's 51 lines: more than two windows
    recs = case["recs"].copy()
    recs["id"]["transport_protocol"][4::5] = 47
    ids = np.full(n, (1 << 64) - 1, dtype=np.uint64)
    ids[1::2] = 1 << 63
    want = splice((line * n, np.arange(n + 1, dtype=np.uint64) * len(line)), recs, ids)
    lens = np.diff(want[1].astype(np.int64))
    assert set(lens.tolist()) == {0, max_line} and (lens[4::5] == 0).all()
    res = N.resolve(case["present"], case["parts"]["network_events"], case["parts"]["drops"], case["answers"]) if ne_table is not None else None
    with tab.tls_names(case["tls"]) as tls, tab.k8s_table(case["k8s"], case["layer"]) as k8s, NC.net_table(nf, case["rules"], tab) as net:
        for got in both_entry_points(nf, tab, tls, k8s, net, recs, ids, case["present"], case["parts"], ne_table, res, names=G.table(nf, case["names"]),
                                     agent=case["agent"], received=case["received"], now=case["now"], mono=case["mono"]):
            KG.check(got, want)
    if ne_table is not None:
        ne_table.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_no_rule_on_gives_the_bytes_of_the_net_encoder_plus_the_keys(nf, O, tab, go_names, netev_table, policy):
    """Against the product's own *_net call rather than the restatement: with every flow tracked, the lines differ by the keys alone."""
    recs, present, parts, answers = TG.policy_inputs(nf, O, 300, 67, policy)
    recs = recs.copy()
    recs["id"]["transport_protocol"] = np.array([6, 17, 132], dtype=np.uint8)[np.arange(300) % 3]
    recs["metrics"]["eth_protocol"] = np.where(np.isin(recs["metrics"]["eth_protocol"], (0x0800, 0x86DD)), recs["metrics"]["eth_protocol"], 0x0800)
    assert tracked(recs).all()
    rows = ne = None
    if answers is not None:
        present, d_out, rows, _, _ = tab.netev_resolve(netev_table, present, parts["network_events"], parts["drops"])
        parts, ne = dict(parts, drops=d_out), netev_table
    names = G.table(nf, NAMES)
    ids = np.arange(300, dtype=np.uint64) << 7
    with tab.k8s_table(KG.entries_for(recs), LAYER) as k8s, tab.net_table(0, NG.CATEGORIES) as off:
        old = tab.encode_flp_json_net(recs, go_names[0], k8s, off, NOW, MONO, names, REPORTER, RECEIVED, present=present, parts=parts, rows=rows, netev_table=ne)
        new = tab.encode_flp_json_conn(recs, go_names[0], k8s, off, ids, NOW, MONO, names, REPORTER, RECEIVED, present=present, parts=parts, rows=rows,
                                       netev_table=ne)
    KG.check(new, splice((old[0].tobytes(), old[1]), recs, ids))
    assert b"SubnetLabel" not in new[0].tobytes() and b"FlowDirection" not in new[0].tobytes() and len(new[0]) > len(old[0]) > 300 * 100


def test_more_than_one_scan_block(nf, O, tab, go_names, netev_table):
    """3000 flows with parts and events: three blocks of the size kernel, 47 waves of the write kernel."""
    recs, present, parts, answers = TG.policy_inputs(nf, O, 3000, 73, 2)
    ids = np.random.default_rng(3).integers(0, 1 << 64, 3000, dtype=np.uint64) >> np.random.default_rng(4).integers(0, 64, 3000).astype(np.uint64)
    want = run(nf, tab, go_names[0], go_names[1], KG.entries_for(recs), LAYER, ALL_WITH_LABELS, recs, ids, present, parts, answers, netev_table)
    keep = tracked(recs)
    assert 300 < keep.sum() < 2700 and want[0].count(b"\n") == int(keep.sum())


def test_argument_checks_with_a_handle(nf, O, tab, go_names):
    import ctypes as C
    recs = G.stream(nf, O, 8, seed=53)
    names = G.table(nf, NAMES)
    L = nf._lib
    with tab.k8s_table([]) as k8s, tab.net_table(7) as net, nf.NetTable(7) as host_only:
        with pytest.raises(nf.NfaggError) as e:
            tab.encode_flp_json_conn(recs, go_names[0], k8s, host_only, np.zeros(8, dtype=np.uint64), NOW, MONO, names, REPORTER, RECEIVED)
        assert e.value.code == L.EINVAL and "net table was not created for this handle" in str(e.value)
        o, keep = nf.flp_options(NOW, MONO, names, REPORTER, RECEIVED)
        off, need = np.zeros(9, dtype=np.uint64), C.c_size_t(7)
        rc = L.lib.nfagg_encode_flp_json_conn(tab._h, recs.ctypes.data_as(C.c_void_p), 8, None, None, None, go_names[0]._t, k8s._t, net._t, None, C.byref(o),
                                              None, 0, off.ctypes.data_as(C.c_void_p), C.byref(need))
        assert rc == L.EINVAL and b"null argument" in L.lib.nfagg_last_error(tab._h)
        d_recs = E.dev(recs)
        with pytest.raises(nf.NfaggError) as e:
            tab.encode_flp_json_conn_device(d_recs.data_ptr(), 8, go_names[0], k8s, net, 0, NOW, MONO, names, REPORTER, RECEIVED, 0, 0, d_recs.data_ptr())
        assert e.value.code == L.EINVAL and "null argument" in str(e.value)
        with pytest.raises(nf.NfaggError) as e:
            tab.encode_flp_json_conn_device(d_recs.data_ptr(), 8, go_names[0], k8s, net, d_recs.data_ptr() + 4, NOW, MONO, names, REPORTER, RECEIVED, 0, 0,
                                            d_recs.data_ptr())
        assert e.value.code == L.EINVAL and "hash ids must be 8-byte aligned" in str(e.value)


# ---- conversation records (nfagg_encode_conn_json): every byte against tests/conn_json_ref.py
import conn_cases as CC  # noqa: E402
import conn_json_ref as CJ  # noqa: E402

ADDRS = ["10.0.0.1", "10.0.1.7", "10.0.2.200", "10.0.3.9", "::ffff:10.0.0.1", "2001:db8::1", "8000::5", "4000:0:0:1::", "192.168.77.1", "::1"]
CONV_ENTRIES = [(a, dict(KG.INFOS[k % len(KG.INFOS)], name="obj-%d" % k)) for k, a in enumerate([ADDRS[0], ADDRS[2], ADDRS[5], ADDRS[6]])]   # ADDRS[4] is ADDRS[0] in its other spelling
EXACT = 1 << 53


def mixed(n, seed):
    """n conversations: every record type, _IsFirst both ways, zero and non-zero aggregates, negative and zero times, 2^53 - 1,
    all address forms, endpoints with and without a Kubernetes row; about one in twenty is deferred (an aggregate of 2^53)."""
    rng = np.random.default_rng(seed)
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    out = []
    for k in range(n):
        big = lambda: pick([0, 0, 1, 7, 12345678901, EXACT - 1])  # noqa: E731
        a, b = pick(ADDRS), pick(ADDRS)
        first = CC.snap(a, b, int(rng.integers(0, 65536)), int(rng.integers(0, 65536)), pick([6, 17, 132]), rng.bytes(6), rng.bytes(6), pick([0x0800, 0x86DD, 0]),
                        int(rng.integers(0, 64)), pick([0, -5, 1_700_000_000_123, -(1 << 62)]), pick([0, 1_700_000_000_456, (1 << 63) - 1]),
                        [int(x) for x in rng.integers(0, 256, int(rng.integers(1, 8)))])
        last = CC.snap(b, a, first["dport"], first["sport"], first["proto"], first["dmac"], first["smac"], 0x0800, 0, 0, 0, [0])
        c = CC.conv(a, b, first["sport"], first["dport"], first["proto"], int(rng.integers(0, 1 << 64, dtype=np.uint64)) >> int(rng.integers(0, 64)),
                    pick(["newConnection", "endConnection", "heartbeat"]), bool(rng.integers(0, 2)), (big(), big()), (big(), big()), (big(), big()),
                    pick([0, -1, -(EXACT - 1), 1_700_000_000_000]), pick([0, 5, EXACT - 1]), first, last)
        if rng.integers(0, 20) == 0:
            c[pick(["flows", "bytes", "packets"])] = pick([(EXACT, 0), (0, EXACT), (EXACT - 1, 1), ((1 << 64) - 1, 0)])
        out.append(c)
    return out


def conv_want(fields, specs, entries, layer, rules):
    table, cats = K.table_of(entries), R.parse_subnets([(R._b(nm), t) for nm, t in (rules.get("labels") or [])])
    lines, deferred = [], []
    for c in specs:
        try:
            lines.append(CJ.line(fields, CC.ref_conv(c), table, layer, rules, cats))
            deferred.append(0)
        except CJ.Deferred:
            lines.append(b"")
            deferred.append(1)
    off = np.cumsum([0] + [len(x) for x in lines]).astype(np.uint64)
    return b"".join(lines), off, np.array(deferred, dtype=np.uint8)


def check_conv(nf, tab, fields, specs, entries=CONV_ENTRIES, layer=LAYER, rules=ALL_WITH_LABELS):
    import torch
    want = conv_want(fields, specs, entries, layer, rules)
    car, val = CC.arrays(nf, specs)
    n = len(specs)
    with tab.conn_layout(fields) as lay, tab.k8s_table(entries, layer) as k8s, NC.net_table(nf, rules, tab) as net:
        G.check(tab.encode_conn_json(car, val, lay, k8s, net), want)
        d_car, d_val = (E.dev(car), E.dev(val)) if n else (None, None)
        args = (d_car.data_ptr() if n else 0, d_val.data_ptr() if n else 0, n, lay, k8s, net)
        d_off = torch.full((n + 1 + 4,), -1, dtype=torch.int64, device="cuda")
        d_def = torch.full((n + 16,), 0xCD, dtype=torch.uint8, device="cuda")
        rc, need, n_def = tab.encode_conn_json_device(*args, 0, 0, d_off.data_ptr())
        assert rc == (nf.TRUNCATED if n else nf.OK) and need == len(want[0]) and n_def == int(want[2].sum())
        d_out = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        if need:
            rc, short, _ = tab.encode_conn_json_device(*args, d_out.data_ptr(), need - 1, d_off.data_ptr(), d_def.data_ptr())
            torch.cuda.synchronize()
            assert rc == nf.TRUNCATED and short == need and bool((d_out == 0xAB).all())
        rc, wrote, n_def = tab.encode_conn_json_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), d_def.data_ptr())
        torch.cuda.synchronize()
        out, off, flags = d_out.cpu().numpy(), d_off.cpu().numpy(), d_def.cpu().numpy()
        assert rc == nf.OK and wrote == need and (out[need:] == 0xAB).all() and (off[n + 1:] == -1).all() and (flags[n:] == 0xCD).all()
        G.check((out[:need], off[:n + 1], flags[:n]), want)
        assert lay.max_line >= int(np.diff(want[1].astype(np.int64)).max(initial=0))
    return want


@pytest.mark.parametrize("fields", ["32 fields", "count only"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 513])
def test_conversation_lines_by_size_and_layout(nf, tab, n, fields):
    want = check_conv(nf, tab, CC.FIELDS_32 if fields == "32 fields" else CC.FIELDS_COUNT, mixed(n, 11 + n))
    if n == 513:
        for text in (b'"_RecordType":"newConnection"', b'"_RecordType":"endConnection"', b'"_RecordType":"heartbeat"', b'"_IsFirst":true', b'"_IsFirst":false',
                     b'"SrcK8S_Name":"obj-', b'"DstSubnetLabel":"', b'"K8S_FlowLayer":"', b'"SrcAddr":"2001:db8::1"', b'"DstAddr":"10.0.0.1"'):
            assert text in want[0], text
        assert 0 < want[2].sum() < n and b"FlowDirection" not in want[0] and b'"Flags"' not in want[0]
        if fields == "32 fields":
            assert b'"TimeFlowStart":-9007199254740991,' in want[0] and b'"DstB":9007199254740991,' in want[0]


def test_zeros_omitted_first_zeros_kept_and_the_edges_of_exactness(nf, tab):
    zero = CC.conv(flows=(0, 0), nbytes=(0, 0), packets=(0, 0), start_min=0, end_max=0, first=CC.snap("::", "::", 0, 0, 0, etype=0), rtype="heartbeat", is_first=False)
    edge = CC.conv(flows=(EXACT - 1, 0), nbytes=(1, EXACT - 2), packets=(0, 5), start_min=-(EXACT - 1), end_max=EXACT - 1, h=(1 << 64) - 1)
    over = [CC.conv(flows=(EXACT, 0)), CC.conv(nbytes=(EXACT - 1, 1)), CC.conv(start_min=-EXACT), CC.conv(end_max=EXACT), CC.conv(packets=(0, 1 << 63))]
    want = check_conv(nf, tab, CC.FIELDS_32, [zero, edge] + over, entries=[], layer=None, rules=R.RULES_OFF)
    lines = want[0].split(b"\n")
    assert want[2].tolist() == [0, 0, 1, 1, 1, 1, 1] and len(lines) == 3
    for absent in (b'"a":', b'"Bytes_', b'"TimeFlowStart":', b'"TimeFlowEnd":', b'"_Foo":', b'"DstB":'):
        assert absent not in lines[0]
    assert b'"DstK8":0,' in lines[0] and b'"SrcK8":"::"' in lines[0] and b'"_HashId":"1","_IsFirst":false,"_RecordType":"heartbeat"' in lines[0]
    assert b'"a":9007199254740991,' in lines[1] and b'"TimeFlowStart":-9007199254740991,' in lines[1] and b'"_HashId":"ffffffffffffffff"' in lines[1]
    # the count-only layout does not look at bytes, packets or times: only the first of the five is deferred
    assert check_conv(nf, tab, CC.FIELDS_COUNT, over, entries=[], layer=None, rules=R.RULES_OFF)[2].tolist() == [1, 0, 0, 0, 0]


@pytest.mark.parametrize("name, lanes", [("lane 0", [0]), ("lane 63", [63]), ("lanes 0 and 63 of two waves", [0, 63, 64, 127]), ("a whole wave", list(range(64, 128))),
                                         ("every conversation", list(range(150)))])
def test_deferred_conversations_by_lane(nf, tab, name, lanes):
    specs = mixed(150, 77)
    for c in specs:
        c["flows"], c["bytes"], c["packets"] = (2, 1), (1000, 10), (3, 4)
    for i in lanes:
        specs[i]["bytes"] = (EXACT, 0)
    want = check_conv(nf, tab, CC.FIELDS_32, specs)
    assert np.flatnonzero(want[2]).tolist() == lanes


@pytest.mark.parametrize("layer", [None, LAYER])
@pytest.mark.parametrize("labels", [False, True])
def test_kubernetes_rows_on_none_one_and_both_sides_and_swapped_endpoints(nf, tab, layer, labels):
    rowed, bare = ADDRS[0], ADDRS[1]
    specs = [CC.conv(a, b, h=k + 1) for k, (a, b) in enumerate([(bare, bare), (rowed, bare), (bare, rowed), (rowed, ADDRS[2]), (ADDRS[2], rowed)])]
    rules = dict(R.RULES_OFF, direction=True, labels=NG.CATEGORIES) if labels else dict(R.RULES_OFF, direction=True)
    want = check_conv(nf, tab, CC.FIELDS_COUNT, specs, layer=layer, rules=rules)[0].split(b"\n")
    assert [(b"SrcK8S_Name" in x, b"DstK8S_Name" in x) for x in want[:5]] == [(False, False), (True, False), (False, True), (True, True), (True, True)]
    assert all((b"K8S_FlowLayer" in x) == (layer is not None) and (b"SubnetLabel" in x) == labels and b"FlowDirection" not in x for x in want[:5])


def test_a_wave_of_conversations_spans_many_windows(nf, tab):
    """Kubernetes rows and labels at their caps on both sides of every conversation, under the 32-field layout."""
    case = NC.worst_case(nf, 1, 0)
    addr = go_ip_text(case["recs"][0]["id"]["src_ip"].tobytes())
    specs = [CC.conv(addr, addr, h=(1 << 64) - 1 - k, flows=(EXACT - 1, 0), nbytes=(EXACT - 1, 0), packets=(EXACT - 1, 0), start_min=-(EXACT - 1), end_max=EXACT - 1,
                     first=CC.snap("1111:2222:3333:4444:5555:6666:7777:8888", "1111:2222:3333:4444:5555:6666:7777:8888", 65535, 65535, 255, b"\xff" * 6, b"\xff" * 6,
                                   65535, 255, -(1 << 63), -(1 << 63), [255] * 7)) for k in range(130)]
    want = check_conv(nf, tab, CC.FIELDS_32, specs, entries=case["k8s"], layer=case["layer"], rules=case["rules"])
    lens = np.diff(want[1].astype(np.int64))
    assert lens.min() > 3000 and 64 * lens.min() > 3 * 16384 and want[0].count(b'SubnetLabel":"\\u0001') == 260


def go_ip_text(b16):
    from flp_json_ref import go_ip
    return go_ip(b16).decode()


def test_conversation_encoder_argument_checks(nf, tab):
    car, val = CC.arrays(nf, [CC.conv()])
    with nf.ConnLayout(CC.FIELDS_COUNT) as host_only, tab.conn_layout(CC.FIELDS_COUNT) as lay, tab.k8s_table([]) as k8s, tab.net_table(0) as net:
        with pytest.raises(nf.NfaggError) as e:
            tab.encode_conn_json(car, val, host_only, k8s, net)
        assert e.value.code == nf._lib.EINVAL and "layout was not created for this handle" in str(e.value)
        with pytest.raises(nf.NfaggError) as e:
            tab.encode_conn_json_device(0, 0, 1, lay, k8s, net, 0, 0, 0)
        assert e.value.code == nf._lib.EINVAL


# ---- ConnTrack.extract_lines: the stage's whole output as bytes, against the restatement's record stream
BIG_PAIR = (("10.0.3.77", 50000), ("10.0.0.78", 443))             # a connection of its own: float64 sums of its bytes are exact


def stage_want(ref, recs, now, tls_ref, table, rules, cats):
    """The bytes behind extract conntrack and transform network for one call: tests/conntrack_ref.py's Extract over the flows'
    maps; a flowLog record is the flow's line of tests/flp_json_net_ref.py with the record's two keys, a conversation record
    goes through the same rules and tests/conn_json_ref.py's marshal. Returns (bytes, conversation records printed with float_f)."""
    net_buf, net_off = R.encode(recs, tls_ref, table, LAYER, rules, T.NOW, T.MONO, G.rows(NAMES), T.AGENT, T.RECEIVED)
    flows = iter(np.flatnonzero(tracked(recs)).tolist())
    lines, n_big = [], 0
    for rec in ref.extract(T.maps(recs), now):
        if rec[b"_RecordType"] == b"flowLog":
            i = next(flows)
            line = net_buf[int(net_off[i]):int(net_off[i + 1])]
            assert line.endswith(b"}\n")
            lines.append(line[:-2] + b',"_HashId":"' + rec[b"_HashId"] + b'","_RecordType":"flowLog"}\n')
            continue
        m = R.apply_rules(dict(rec), table, LAYER, rules, cats)
        try:
            lines.append(CJ.marshal(m) + b"\n")
        except CJ.Deferred:
            lines.append(CJ.marshal(m, defer=False) + b"\n")
            n_big += 1
    assert "flowLog" not in ref.out_types or next(flows, None) is None
    return b"".join(lines), n_big


@pytest.mark.parametrize("flow_logs", [True, False])
def test_extract_lines_over_four_calls_against_the_restatement(nf, tab, go_names, flow_logs):
    """600 flows in four calls with a moving clock: newConnection, flowLog, heartbeat and endConnection records, two scheduling
    groups, a connection limit below the stream's connection count, ICMP flows that leave no line, Kubernetes rows, the layer
    and subnet labels on flows and conversations alike. One connection carries 2^60 bytes in its first call and 3 * 2^59 more
    in its second: each of its conversation records is deferred by the device and formatted on the host."""
    rng = np.random.default_rng(21)
    ends = [("10.0.%d.%d" % (k % 4, k + 1), 1000 + k) for k in range(24)] + [("2001:db8::%x" % k, 80 + 100 * k) for k in range(1, 9)] + \
           [("8000::%x" % k, 443) for k in range(1, 9)]
    cfg = T.config(max_conns=60, flow_logs=flow_logs)
    ref, mir = CT.ConnTrack(cfg), nf.ConnTrack(cfg)
    entries = [(a, dict(KG.INFOS[k % len(KG.INFOS)], name="obj-%d" % k)) for k, a in enumerate([e[0] for e in ends[::3]] + [BIG_PAIR[0][0]])]
    rules = ALL_WITH_LABELS
    table, cats = K.table_of(entries), R.parse_subnets([(R._b(nm), t) for nm, t in rules["labels"]])
    now, n_big, whole = 0, 0, []
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, rules, tab) as net, mir.layout(tab) as lay:
        for call in range(4):
            flows = []
            for _ in range(150):
                lo, n_ends = (0, 24) if rng.integers(0, 2) else (24, 16)
                a, b = rng.choice(n_ends, 2, replace=False)
                flows.append(dict(src=ends[lo + a][0], sport=ends[lo + a][1], dst=ends[lo + b][0], dport=ends[lo + b][1],
                                  proto=int(rng.choice([6, 6, 6, 17, 17, 132, 1])), bytes=int(rng.integers(0, 1 << 40)) * int(rng.integers(0, 4) > 0),
                                  packets=int(rng.integers(0, 1000)), flags=int(rng.choice([0, 0x10, 0x10, 0x11, 0x112, 0x01, 0x02]))))
            if call < 2:
                (a, ap), (b, bp) = BIG_PAIR if call == 0 else BIG_PAIR[::-1]
                flows[40 + call] = dict(src=a, sport=ap, dst=b, dport=bp, proto=6, bytes=(1 << 60) if call == 0 else 3 << 59, packets=9, flags=0x10)
            now += int(rng.integers(2 * 10**9, 5 * 10**9))
            recs = T.records(nf, flows)
            want, big = stage_want(ref, recs, now, go_names[1], table, rules, cats)
            got = mir.extract_lines(tab, recs, now, T.NOW, T.MONO, G.table(nf, NAMES), go_names[0], k8s, net, agent_ip=T.AGENT, time_received=T.RECEIVED,
                                    layout=lay if call % 2 else None, cap=64)                               # cap 64: the fold's cap grows
            if got != want:
                g, w = got.split(b"\n"), want.split(b"\n")
                k = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
                raise AssertionError("call %d, line %d of %d / %d:\n got %r\nwant %r" % (call, k, len(g), len(w), g[k:k + 1], w[k:k + 1]))
            n_big += big
            whole.append(want)
            assert len(mir) == len(ref.group_of)
    out = b"".join(whole)
    for text in (b'"_RecordType":"newConnection"', b'"_RecordType":"endConnection"', b'"_RecordType":"heartbeat"', b'"_IsFirst":false', b'"SrcK8S_Name":"obj-',
                 b'"DstSubnetLabel":"', b'"K8S_FlowLayer":"', b'"Bytes_AB":1152921504606847000,', b'"numFlowLogs":2}'):
        assert text in out, text
    assert (b'"_RecordType":"flowLog"' in out) == flow_logs and n_big >= 2
    # the deferred connection after its second call: 2^60 one way, 3 * 2^59 the other, each with the shortest digits and zeros
    assert any(b'"Bytes_AB":1152921504606847000,"Bytes_BA":1729382256910270500,' in x and b'"_RecordType":"newConnection"' not in x for x in out.split(b"\n"))
