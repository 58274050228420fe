"""direct-FLP JSON with direction, subnet labels and TCP flag names on the GPU (nfagg_encode_flp_json_net, nfagg_net_resolve;
csrc/nfagg_net.h, nfagg_net.hip) through the C ABI, host and device entry points, all three policies: every byte and every
offset against the restatement of tests/flp_json_net_ref.py, the resolved rows against plain Python. Records, namer table,
parts, network events and informer answers are those of the Kubernetes tests."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_k8s_ref as K  # noqa: E402
import flp_json_net_ref as R  # noqa: E402
import flp_json_tls_ref as T  # noqa: E402
import netev_ref as N  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_flp_json_k8s_gpu as KG  # noqa: E402
import test_flp_json_net_cpu as NC  # noqa: E402
import test_flp_json_tls_gpu as TG  # noqa: E402
import test_netev_gpu as E  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, NOW, MONO, RECEIVED = G.NAMES, G.NOW, G.MONO, G.RECEIVED
POLICIES = (0, 1, 2)
GOLDEN = NC.GOLDEN
LAYER, INFOS, check = KG.LAYER, KG.INFOS, KG.check
REPORTER = bytes(10) + b"\xff\xff" + bytes([192, 168, 1, 10])      # INFOS[0]'s host IP: some of a stream's flows leave or reach the reporter
# first match, not longest prefix: the streams' IPv4 addresses are 10.0.{0..3}.x; a /23 stands ahead of a /24 inside it, an empty
# name ahead of the /24 that holds its /25, and the halves of IPv6 ahead of a /32
CATEGORIES = [("low v4", ["10.0.0.0/23"]), ("", ["10.0.2.0/25"]), ("high v4", ["10.0.2.0/24", "10.0.3.0/24"]), (INFOS[5]["owner_name"], ["::/2", "4000::/2"]),
              ("high v6", ["8000::/1"]), ("never", ["10.0.1.0/24", "2001:db8::/32"])]
ALL = dict(direction=True, labels=CATEGORIES, flags=True)
RULE_SETS = {"direction": dict(R.RULES_OFF, direction=True), "labels": dict(R.RULES_OFF, labels=CATEGORIES), "flags": dict(R.RULES_OFF, flags=True), "all": ALL}


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


def both_entry_points(nf, tab, tls, k8s, net, recs, present, parts, ne_table, want_resolve, names=None, agent=REPORTER, received=RECEIVED, now=NOW, mono=MONO):
    """The host call and the device call, with the protocol of test_flp_json_k8s_gpu.both_entry_points: the size query, a buffer
    one byte short (NFAGG_TRUNCATED, nothing written), then the write into a buffer with canaries behind it."""
    import torch
    names = names if names is not None else G.table(nf, NAMES)
    n = len(recs)
    rows = None
    if ne_table is not None:
        present, d_out, rows, missing, _ = tab.netev_resolve(ne_table, present, parts["network_events"], parts["drops"])
        assert set(missing) == want_resolve[4] and rows.tolist() == want_resolve[2].tolist()
        parts = dict(parts, drops=d_out)
    host = tab.encode_flp_json_net(recs, tls, k8s, net, now, mono, names, agent, received, present=present, parts=parts, rows=rows, netev_table=ne_table)
    d_recs = E.dev(recs) if n else None
    d_present = E.dev(present) if present is not None and n else None
    d_parts = {k: E.dev(v) for k, v in (parts or {}).items() if k != "network_events"} if n else {}
    d_rows = E.dev(rows) if rows is not None and n else None
    kw = dict(d_present=d_present.data_ptr() if d_present is not None else 0, d_parts={k: v.data_ptr() for k, v in d_parts.items()},
              d_rows=d_rows.data_ptr() if d_rows is not None else 0, netev_table=ne_table if d_rows is not None else None)
    args = (d_recs.data_ptr() if n else 0, n, tls, k8s, net, now, mono, names, agent, received)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    rc, need = tab.encode_flp_json_net_device(*args, 0, 0, d_off.data_ptr(), **kw)
    assert rc == (nf.TRUNCATED if n else nf.OK) and need == len(host[0])               # the size query: the exact byte count
    d_out = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    if n:
        rc, short = tab.encode_flp_json_net_device(*args, d_out.data_ptr(), need - 1, d_off.data_ptr(), **kw)
        torch.cuda.synchronize()
        assert rc == nf.TRUNCATED and short == need and bool((d_out == 0xAB).all())
    rc, wrote = tab.encode_flp_json_net_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), **kw)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert rc == nf.OK and wrote == need and (out[need:] == 0xAB).all()
    return host, (out[:need], d_off.cpu().numpy())


def run(nf, tab, tls, tls_ref, entries, layer, rules, recs, present=None, parts=None, answers=None, ne_table=None, agent=REPORTER):
    events = res = None
    rp, rparts = present, parts
    if answers is not None:
        res = N.resolve(present, parts["network_events"], parts["drops"], answers)
        rp, rparts, events = res[0], dict(parts, drops=res[1]), res[3]
    want = R.encode(recs, tls_ref, K.table_of(entries), layer, rules, NOW, MONO, G.rows(NAMES), agent, RECEIVED, present=rp, parts=rparts, events=events)
    with tab.k8s_table(entries, layer) as k8s, NC.net_table(nf, rules, tab) as net:
        for got in both_entry_points(nf, tab, tls, k8s, net, recs, present, parts, ne_table if answers is not None else None, res, agent=agent):
            check(got, want)
    return want


def resolve_rows(got):
    return list(zip(got["src_label"].tolist(), got["dst_label"].tolist(), got["direction"].tolist()))


def ip_records(nf, pairs, proto=6, eth=None):
    """One record per (src, dst) pair of addresses given as text or 16 bytes."""
    recs = np.zeros(len(pairs), dtype=nf.FLOW_RECORD)
    for i, (s, d) in enumerate(pairs):
        s, d = K.ip16(s), K.ip16(d)
        recs["id"]["src_ip"][i], recs["id"]["dst_ip"][i] = np.frombuffer(s, dtype=np.uint8), np.frombuffer(d, dtype=np.uint8)
        recs["metrics"]["eth_protocol"][i] = 0x0800 if s[:12] == R.V4_IN_V6 else 0x86DD
    if eth is not None:
        recs["metrics"]["eth_protocol"] = eth
    recs["id"]["transport_protocol"] = proto
    recs["id"]["src_port"], recs["id"]["dst_port"] = 40000, 443
    recs["metrics"]["bytes"], recs["metrics"]["packets"], recs["metrics"]["flags"] = 1500, 3, 0x12
    return recs


@pytest.fixture(scope="module")
def stream_entries(nf, O):
    return KG.entries_for(TG.policy_inputs(nf, O, 257, 61, 0)[0])


# ---- rules on and off, shapes
@pytest.mark.parametrize("policy", POLICIES)
def test_no_rule_on_gives_the_bytes_of_the_k8s_encoder(nf, O, tab, go_names, netev_table, policy):
    recs, present, parts, answers = TG.policy_inputs(nf, O, 300, 67, policy)
    rows = ne = None
    if answers is not None:
        present, d_out, rows, _, _ = tab.netev_resolve(netev_table, present, parts["network_events"], parts["drops"])
        parts, ne = dict(parts, drops=d_out), netev_table
    names = G.table(nf, NAMES)
    with tab.k8s_table(KG.entries_for(recs), LAYER) as k8s, tab.net_table(0, CATEGORIES) as off:
        old = tab.encode_flp_json_k8s(recs, go_names[0], k8s, NOW, MONO, names, REPORTER, RECEIVED, present=present, parts=parts, rows=rows, netev_table=ne)
        new = tab.encode_flp_json_net(recs, go_names[0], k8s, off, NOW, MONO, names, REPORTER, RECEIVED, present=present, parts=parts, rows=rows, netev_table=ne)
    assert old[0].tobytes() == new[0].tobytes() and old[1].tolist() == new[1].tolist() and len(old[0]) > 300 * 100
    assert b"SubnetLabel" not in new[0].tobytes() and b"FlowDirection" not in new[0].tobytes() and b'"Flags":[' not in new[0].tobytes()


@pytest.mark.parametrize("rules", list(RULE_SETS))
@pytest.mark.parametrize("policy", POLICIES)
def test_each_rule_alone_and_all_together(nf, O, tab, go_names, netev_table, stream_entries, policy, rules):
    recs, present, parts, answers = TG.policy_inputs(nf, O, 257, 61, policy)
    want = run(nf, tab, go_names[0], go_names[1], stream_entries, LAYER, RULE_SETS[rules], recs, present, parts, answers, netev_table)[0]
    has = {"direction": (b'"FlowDirection":0', b'"FlowDirection":1', b'"FlowDirection":2'), "flags": (b'"Flags":[', b'"Flags":null'),
           "labels": (b'"SrcSubnetLabel":"low v4"', b'"DstSubnetLabel":"high v4"', b'"SrcSubnetLabel":"q\\"b\\\\\\t', b'"DstSubnetLabel":"high v6"')}
    for name, texts in has.items():
        for text in texts:
            assert (text in want) == (rules in (name, "all")), (name, text)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("policy", POLICIES)
def test_record_counts_policies_and_entry_points(nf, O, tab, go_names, netev_table, stream_entries, policy, n):
    recs, present, parts, answers = TG.policy_inputs(nf, O, 257, 61, policy)
    cut = lambda a: a[:n] if a is not None else None  # noqa: E731
    want = run(nf, tab, go_names[0], go_names[1], stream_entries, LAYER, ALL, recs[:n], cut(present), {k: v[:n] for k, v in parts.items()} if parts else parts,
               answers, netev_table)
    assert len(want[1]) == n + 1 and want[0].count(b'"K8S_FlowLayer":"') == n


def worst_inputs(nf, tab, n, policy):
    case = NC.worst_case(nf, n, policy)
    one = {**case, "recs": case["recs"][:1], "present": case["present"][:1] if case["present"] is not None else None,
           "parts": {k: v[:1] for k, v in case["parts"].items()} if case["parts"] else None}
    line, _ = NC.reference(one)
    ne_table = tab.netev_table(case["answers"].items()) if case["answers"] is not None else None
    return case, line, ne_table


@pytest.mark.parametrize("policy", POLICIES)
def test_a_wave_spans_many_windows_and_every_line_is_the_longest(nf, tab, policy):
    """130 flows at the policy's worst case: every line has exactly the bytes the write kernel sizes its window by, so the first
    two waves take a window for every one or two lines and the last wave is partial."""
    n = 130
    case, line, ne_table = worst_inputs(nf, tab, n, policy)
    max_line = nf._lib.lib.nfagg_flp_json_net_max_line(policy)
    window = (32768 - (16 if policy == 0 else 2048) - (max_line + 15) // 16 * 16) // 16 * 16       # FlpNet<Base>::kWindow
    assert len(line) == max_line and 64 * max_line > 20 * window
    want = (line * n, np.arange(n + 1, dtype=np.uint64) * max_line)                                # every record is the same flow
    res = N.resolve(case["present"], case["parts"]["network_events"], case["parts"]["drops"], case["answers"]) if ne_table is not None else None
    with tab.tls_names(case["tls"]) as tls, tab.k8s_table(case["k8s"], case["layer"]) as k8s, NC.net_table(nf, case["rules"], tab) as net:
        for got in both_entry_points(nf, tab, tls, k8s, net, case["recs"], case["present"], case["parts"], ne_table, res, names=G.table(nf, case["names"]),
                                     agent=case["agent"], received=case["received"], now=case["now"], mono=case["mono"]):
            check(got, want)
    if ne_table is not None:
        ne_table.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_a_stream_that_mixes_worst_case_and_short_lines(nf, tab, policy):
    """Every third flow is the policy's worst case, the others carry no part, no row and no label (445 bytes, most of them the
    worst case's agent address and times): windows of one long line and many short ones."""
    n = 200
    case, line, ne_table = worst_inputs(nf, tab, n, policy)
    recs = case["recs"].copy()
    short = np.arange(n) % 3 != 0
    small = ip_records(nf, [("10.9.8.7", "10.9.8.6")])[0]
    recs[short] = small
    present = case["present"]
    if present is not None:
        present = present.copy()
        present[short] = 0
    rules = dict(NC.ALL, labels=[(NC.CAP_LABEL, ["1000::/4"])])                                      # holds the worst flow's address, no IPv4 one
    case = {**case, "recs": recs, "present": present, "rules": rules}
    want = NC.reference(case)
    lens = np.diff(want[1].astype(np.int64))
    assert lens[0] == len(line) and lens[::3].min() == len(line) and 250 < lens[short].min() and lens[short].max() < 450
    res = N.resolve(present, case["parts"]["network_events"], case["parts"]["drops"], case["answers"]) if ne_table is not None else None
    with tab.tls_names(case["tls"]) as tls, tab.k8s_table(case["k8s"], case["layer"]) as k8s, NC.net_table(nf, rules, tab) as net:
        for got in both_entry_points(nf, tab, tls, k8s, net, recs, present, case["parts"], ne_table, res, names=G.table(nf, case["names"]),
                                     agent=case["agent"], received=case["received"], now=case["now"], mono=case["mono"]):
            check(got, want)
    if ne_table is not None:
        ne_table.close()


# ---- reinterpret_direction
HOST_A, HOST_B, HOST_R = "192.168.7.1", "192.168.7.2", "192.168.7.9"
STATES = ("no row", "empty host IP", "A", "B", "reporter")


def direction_world(host_r=HOST_R):
    """Two addresses per state (so that src and dst can share a host and still differ), the informer answers behind them."""
    addr = {s: ("10.50.%d.1" % k, "10.50.%d.2" % k) for k, s in enumerate(STATES)}
    host = {"empty host IP": "", "A": HOST_A, "B": HOST_B, "reporter": host_r}
    entries = [(ip, dict(namespace="shop", name="pod-%s-%d" % (s[:1], k), kind="Pod", host_ip=host[s], host_name="node"))
               for s in STATES[1:] for k, ip in enumerate(addr[s])]
    return addr, entries


def matrix_want(s, d):
    if s in ("no row", "empty host IP") and d in ("no row", "empty host IP"):
        return None
    if s == d:
        return 2
    return 1 if s == "reporter" else 0 if d == "reporter" else None


def test_direction_matrix(nf, tab, go_names):
    """src and dst host over {no row, row with an empty host IP, A, B, the reporter}; on the diagonal two rows with the same host IP."""
    addr, entries = direction_world()
    cells = [(s, d) for s in STATES for d in STATES]
    recs = ip_records(nf, [(addr[s][0], addr[d][1]) for s, d in cells])
    rules = dict(R.RULES_OFF, direction=True)
    agent = K.ip16(HOST_R)
    want = run(nf, tab, go_names[0], go_names[1], entries, LAYER, rules, recs, agent=agent)[0].split(b"\n")
    for (s, d), line in zip(cells, want):
        w = matrix_want(s, d)
        assert (b'"FlowDirection":%d,' % w in line) if w is not None else (b"FlowDirection" not in line), (s, d)
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, rules, tab) as net:
        got = tab.net_resolve(net, recs, k8s, tab.k8s_resolve(k8s, recs), agent)
    assert resolve_rows(got) == R.resolve(recs, entries, rules, agent) == [(R.NO_LABEL, R.NO_LABEL, R.NO_DIRECTION if matrix_want(s, d) is None else matrix_want(s, d))
                                                                           for s, d in cells]


@pytest.mark.parametrize("name, agent, host_r, only", [
    ("a reporter no row has", "192.168.7.200", HOST_R, {2}),
    ("a nil agent address", None, HOST_R, {2}),
    ("a nil agent address and a row whose host IP text is <nil>", None, "<nil>", {0, 1, 2}),
    ("an IPv6 agent, the host IP in the text the line prints", "fd00::1:0:0:9", "fd00::1:0:0:9", {0, 1, 2}),
    ("an IPv6 agent, the host IP in another spelling", "fd00::1:0:0:9", "fd00:0:0:0:1::9", {2}),
    ("a v4-mapped agent, the host IP dotted", "::ffff:192.168.7.9", HOST_R, {0, 1, 2}),
])
def test_direction_by_text_identity(nf, tab, go_names, name, agent, host_r, only):
    addr, entries = direction_world(host_r)
    cells = [(s, d) for s in STATES for d in STATES]
    recs = ip_records(nf, [(addr[s][0], addr[d][1]) for s, d in cells])
    agent = K.ip16(agent) if agent is not None else None
    want = run(nf, tab, go_names[0], go_names[1], entries, None, dict(R.RULES_OFF, direction=True), recs, agent=agent)[0]
    assert {k for k in (0, 1, 2) if b'"FlowDirection":%d' % k in want} == only, name
    assert (b'"AgentIP":"<nil>"' in want) == (agent is None)


def test_direction_without_ip_and_without_rows(nf, tab, go_names):
    addr, entries = direction_world()
    pairs = [(addr["reporter"][0], addr["A"][0]), (addr["A"][0], addr["A"][1])]
    recs = np.concatenate([ip_records(nf, pairs), ip_records(nf, pairs, eth=0x0806), ip_records(nf, pairs, eth=0)])
    rules = dict(R.RULES_OFF, direction=True)
    agent = K.ip16(HOST_R)
    lines = run(nf, tab, go_names[0], go_names[1], entries, LAYER, rules, recs, agent=agent)[0].split(b"\n")
    assert b'"FlowDirection":1' in lines[0] and b'"FlowDirection":2' in lines[1] and all(b"FlowDirection" not in x for x in lines[2:])
    assert b"FlowDirection" not in run(nf, tab, go_names[0], go_names[1], [], LAYER, rules, recs, agent=agent)[0]      # an empty Kubernetes table


# ---- add_subnet_label
def vector_ips():
    return sorted({c["ip"] for c in GOLDEN["contains"]})


def test_containment_vectors_on_the_device(nf, tab):
    """Every CIDR of tests/golden/net_vectors.json as a table of its own against every address of the file: the prefixes 0, 1, 13,
    31, 32 and 0, 1, 77, 127, 128, ::ffff:10.0.0.0/104 as 10.0.0.0/8, ::/0 and 0.0.0.0/0 each blind to the other family."""
    ips = vector_ips()
    recs = ip_records(nf, list(zip(ips, reversed(ips))))
    cidrs = sorted({c["cidr"] for c in GOLDEN["contains"]})
    for want_len in ("/0", "/1", "/13", "/31", "/32", "/77", "/127", "/128", "/104"):
        assert any(c.endswith(want_len) for c in cidrs)
    for cidr in cidrs:
        rules = dict(R.RULES_OFF, labels=[("hit", [cidr])])
        with NC.net_table(nf, rules, tab) as net:
            got = resolve_rows(tab.net_resolve(net, recs))
        assert got == R.resolve(recs, [], rules, None), cidr
        for c in GOLDEN["contains"]:
            if c["cidr"] == cidr:
                assert got[ips.index(c["ip"])][0] == (0 if c["want"] else R.NO_LABEL), c


def test_first_match_empty_name_escapes_and_the_cap(nf, tab, go_names):
    cats = [(NC.latin(n), t) for n, t in GOLDEN["labels"]["categories"]] + [(INFOS[5]["owner_name"], ["9.0.0.0/8"]), (NC.CAP_LABEL, ["2001:dead::/32"])]
    ips = [c["ip"] for c in GOLDEN["labels"]["cases"]] + ["9.9.4.4", "2001:dead::77"]
    recs = np.concatenate([ip_records(nf, list(zip(ips, reversed(ips)))), ip_records(nf, [("10.1.2.3", "10.1.2.3")], eth=0x0806)])
    rules = dict(R.RULES_OFF, labels=cats)
    want = run(nf, tab, go_names[0], go_names[1], [], None, rules, recs)[0]
    lines = want.split(b"\n")
    for k, c in enumerate(GOLDEN["labels"]["cases"]):
        frag = R.render(NC.latin(c["want"]), 0)
        assert (frag in lines[k]) if frag else (b"SrcSubnetLabel" not in lines[k]), c
    assert b'"SrcSubnetLabel":"broad"' in lines[0] and b"narrow" not in want                       # the broad CIDR stands first
    assert R.render(INFOS[5]["owner_name"], 1) in want and R.render(NC.CAP_LABEL, 0) in want and b"SubnetLabel" not in lines[len(ips)]
    with NC.net_table(nf, rules, tab) as net:
        got = resolve_rows(tab.net_resolve(net, recs))
    assert got == R.resolve(recs, [], rules, None) and got[2][0] == 2 and got[len(ips)] == (R.NO_LABEL, R.NO_LABEL, R.NO_DIRECTION)


def test_zero_cidrs_and_the_list_at_its_cap(nf, tab, go_names):
    recs = ip_records(nf, [("10.200.0.1", "fd00::1"), ("fd00::1", "10.200.0.2"), ("9.9.9.9", "9.9.9.9")])
    want = run(nf, tab, go_names[0], go_names[1], [], None, dict(R.RULES_OFF, labels=[]), recs)[0]
    assert b"SubnetLabel" not in want
    # 1 024 CIDRs, the only one that holds an address of the records last
    miss = ["172.%d.%d.0/24" % (16 + k // 256, k % 256) for k in range(1000)] + ["2001:db8:%x::/48" % k for k in range(23)]
    rules = dict(R.RULES_OFF, labels=[("miss", miss), ("last", ["10.200.0.0/31"])])
    with NC.net_table(nf, rules, tab) as net:
        assert net.n_cidrs == nf._lib.NET_MAX_CIDRS
        got = resolve_rows(tab.net_resolve(net, recs))
    assert got == [(1, R.NO_LABEL, R.NO_DIRECTION), (R.NO_LABEL, R.NO_LABEL, R.NO_DIRECTION), (R.NO_LABEL, R.NO_LABEL, R.NO_DIRECTION)]
    want = run(nf, tab, go_names[0], go_names[1], [], None, rules, recs)[0]
    assert want.count(b'"SrcSubnetLabel":"last"') == 1 and want.count(b"SubnetLabel") == 1


# ---- decode_tcp_flags
def test_flag_sweep(nf, tab, go_names):
    """All 2 048 values of the low eleven bits on protocol-6 records, then 0xF800, 0xFFFF, and protocols 17 and 1, which have no
    Flags key."""
    values = list(range(2048)) + [0xF800, 0xFFFF, 0x12, 0x12]
    recs = ip_records(nf, [("10.0.0.1", "10.0.0.2")] * len(values))
    recs["metrics"]["flags"] = values
    recs["id"]["transport_protocol"][-2:] = [17, 1]
    want = run(nf, tab, go_names[0], go_names[1], [], None, dict(R.RULES_OFF, flags=True), recs)[0]
    lines = want.split(b"\n")
    every = b'"Flags":["FIN","SYN","RST","PSH","ACK","URG","ECE","CWR","SYN_ACK","FIN_ACK","RST_ACK"],'
    assert b'"Flags":null,' in lines[0] and b'"Flags":null,' in lines[2048] and every in lines[2047] and every in lines[2049]
    assert b"Flags" not in lines[2050] and b"Flags" not in lines[2051] and want.count(b'"Flags":') == 2050
    for c in GOLDEN["flags"]:
        if c["value"] < 2048:
            text = b"null" if c["want"] is None else b"[" + b",".join(b'"%s"' % x.encode() for x in c["want"]) + b"]"
            assert b'"Flags":' + text + b"," in lines[c["value"]]


# ---- the join alone
def test_resolve_against_python_host_and_device(nf, O, tab):
    import torch
    recs = G.stream(nf, O, 3000, seed=71)
    entries = KG.entries_for(recs, every=2)
    want = R.resolve(recs, entries, ALL, REPORTER)
    dirs = {d for _, _, d in want}
    labels = {s for s, _, _ in want} | {d for _, d, _ in want}
    assert dirs == {0, 1, 2, R.NO_DIRECTION} and labels >= {0, 1, 2, 3, 4, R.NO_LABEL} and 5 not in labels
    with tab.k8s_table(entries) as k8s, NC.net_table(nf, ALL, tab) as net, NC.net_table(nf, R.RULES_OFF, tab) as off:
        k8s_rows = tab.k8s_resolve(k8s, recs)
        assert resolve_rows(tab.net_resolve(net, recs, k8s, k8s_rows, REPORTER)) == want
        assert len(tab.net_resolve(net, recs[:0], k8s, k8s_rows[:0], REPORTER)) == 0
        assert set(resolve_rows(tab.net_resolve(off, recs))) == {(R.NO_LABEL, R.NO_LABEL, R.NO_DIRECTION)}
        d_recs, d_k8s = E.dev(recs), E.dev(k8s_rows)
        d_out = torch.full((len(recs) + 4, 2), 0x55555555, dtype=torch.int32, device="cuda")
        tab.net_resolve_device(net, d_recs.data_ptr(), len(recs), d_out.data_ptr(), k8s, d_k8s.data_ptr(), REPORTER)
        raw = d_out.cpu().numpy()
        got = raw[:len(recs)].copy().view(nf.NET_ROW).reshape(-1)
        assert resolve_rows(got) == want and (got["pad_"] == 0).all() and (raw[len(recs):] == 0x55555555).all()
        with pytest.raises(nf.NfaggError) as e:
            tab.net_resolve(net, recs)                                                 # direction on, no Kubernetes rows
        assert e.value.code == nf._lib.EINVAL and "reinterpret_direction needs" in str(e.value)


def test_more_than_one_scan_block(nf, O, tab, go_names, netev_table):
    """3000 flows with parts and events: three blocks of the size kernel, 47 waves of the write kernel."""
    recs, present, parts, answers = TG.policy_inputs(nf, O, 3000, 73, 2)
    want = run(nf, tab, go_names[0], go_names[1], KG.entries_for(recs), LAYER, ALL, recs, present, parts, answers, netev_table)
    assert want[0].count(b'"SrcSubnetLabel"') > 300 and want[0].count(b'"FlowDirection"') > 100 and want[0].count(b'"Flags":[') > 100


def test_argument_checks_with_a_handle(nf, O, tab, go_names):
    recs = G.stream(nf, O, 8, seed=53)
    names = G.table(nf, NAMES)
    with tab.k8s_table([]) as k8s, nf.NetTable(7) as host_only:
        with pytest.raises(nf.NfaggError) as e:
            tab.encode_flp_json_net(recs, go_names[0], k8s, host_only, NOW, MONO, names, REPORTER, RECEIVED)
        assert e.value.code == nf._lib.EINVAL and "net table was not created for this handle" in str(e.value)
        with pytest.raises(nf.NfaggError) as e:
            tab.net_resolve(host_only, recs, k8s, np.zeros((8, 2), dtype=np.uint32), REPORTER)
        assert e.value.code == nf._lib.EINVAL and "net table was not created for this handle" in str(e.value)
    with nf.K8sTable([]) as host_k8s, tab.net_table(7) as net:
        with pytest.raises(nf.NfaggError) as e:
            tab.encode_flp_json_net(recs, go_names[0], host_k8s, net, NOW, MONO, names, REPORTER, RECEIVED)
        assert e.value.code == nf._lib.EINVAL and "Kubernetes table was not created for this handle" in str(e.value)


def test_exporter_and_map_tracer_with_the_rules(nf, O, tab, go_names):
    recs = G.stream(nf, O, 700, seed=79, keep_tls=True)
    entries = KG.entries_for(recs)
    out = io.BytesIO()
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, ALL, tab) as net:
        exp = nf.StartDirectFLPJSON(tab, out, names=G.table(nf, NAMES), agent_ip=REPORTER, time_received=lambda: RECEIVED, tls_names=go_names[0], k8s=k8s,
                                    net=net)
        assert exp.ExportEvicted(recs[:400], NOW, MONO) == 400 and exp.ExportEvicted(recs[400:], NOW, MONO) == 300
    want = R.encode(recs, go_names[1], K.table_of(entries), LAYER, ALL, NOW, MONO, G.rows(NAMES), REPORTER, RECEIVED)[0]
    assert out.getvalue() == want and want.count(b'"FlowDirection"') > 20 and (exp.lines, exp.deferred) == (700, 0)

    from test_map_merge import make_maps
    n_cpu = 4
    main_ids, main_vals, feats = make_maps(O, seed=11, n_pop=400, n_main=300, n_feat=250, n_cpu=n_cpu)
    main_vals["eth_protocol"] = 0x86DD                                        # the maps' random ethertypes would leave no address key
    drained = (main_ids, main_vals, feats, n_cpu)
    decoder = lambda cookie: None if cookie[0] % 2 == 0 else b"event %d" % cookie[1]  # noqa: E731
    mrecs, present, parts, _ = tab.map_merge(main_ids, main_vals, feats, n_cpu)
    entries = KG.entries_for(mrecs)
    (wp, wd, wrows, events, _), answers, _ = N.resolve_loop(present, parts["network_events"], parts["drops"], decoder)
    want = R.encode(mrecs, go_names[1], K.table_of(entries), LAYER, ALL, NOW, MONO, G.rows(NAMES), REPORTER, RECEIVED, present=wp, parts=dict(parts, drops=wd),
                    events=events)
    mt = nf.MapTracer(nf.GPUMapFetcher(tab, lambda: drained), 0, 0, sample_decoder=decoder, clock=lambda: NOW, mono_clock=lambda: MONO)
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, ALL, tab) as net:
        check(mt.evictFlowsJSON(G.table(nf, NAMES), REPORTER, RECEIVED, tls_names=go_names[0], k8s=k8s, net=net), want)
    assert any(events) and b'SubnetLabel":"' in want[0] and b'"NetworkEvents":[' in want[0]
