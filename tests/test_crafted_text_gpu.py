"""The battery of tests/textcraft.py (addresses by zero / non-zero pattern and width class, decimal edges of every numeric field, clock
cases with both carries, conntrack ids of every hex width) through every line kernel pair, host and device entry points: nfagg_encode_flp_json,
_content, _netev, _tls / _k8s / _net / _conn in their three policies, nfagg_encode_conn_json; the clocks and digits families through the
protobuf and IPFIX encoders as well. Three arrangements: interleaved (neighbouring lanes differ), grouped (whole waves of one family), odd
lane (one battery record among 63 plain ones). Expected bytes: the restatements the seeded-stream tests of each encoder already use
(tests/test_textcraft_cpu.py holds them against ipaddress, str(int) and floor division on this battery); the entry-point protocols (size query,
one byte short, canaries, offsets) are those tests' own helpers.

Sensitivity, observed once on an MI355X with the library rebuilt from a scratch copy carrying one changed token (each changes the size pass
and the write pass alike). "old" is tests/test_flp_json_gpu.py without its one-million-flow test, 16 tests:

  mutant                                                     this file (73 tests)   old
  ip_text: `curlen > zlen` -> `>=`                           57 fail                10 fail (a lone zero group becomes "::" too: gross)
  ndigits, 32-bit arm: `x >= p` -> `>` (dec<3|5|10>)         57 fail                13 fail (an octet or port of 10 or 100 is common)
  ndigits, 64-bit arm: `v >= p` -> `>` (dec<20>, dec_i64)    56 fail                all pass
  flow_time: `nsec >= 1000000000ll` -> `>`                   10 fail                all pass

The flow_time mutant leaves every JSON line as it is: with nsec = 10^9 kept, sec * 1000 + nsec / 10^6 is the same number of milliseconds. It
shows where seconds and nanoseconds travel apart: the ten failures are the protobuf and IPFIX tests of the five calls whose now_nsec is not 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conn_cases as CC  # noqa: E402
import flp_json_content_ref as RC  # noqa: E402
import flp_json_k8s_ref as K  # noqa: E402
import flp_json_net_ref as RN  # noqa: E402
import flp_json_ref as R  # noqa: E402
import flp_json_tls_ref as T  # noqa: E402
import ipfix_ref as IR  # noqa: E402
import netev_ref as N  # noqa: E402
import test_conn_lines_gpu as CL  # noqa: E402
import test_export_edges_gpu as XE  # noqa: E402
import test_flp_json_content_gpu as CG  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_flp_json_k8s_gpu as KG  # noqa: E402
import test_flp_json_net_cpu as NC  # noqa: E402
import test_flp_json_net_gpu as NG  # noqa: E402
import test_flp_json_tls_gpu as TG  # noqa: E402
import test_netev_gpu as E  # noqa: E402
import test_pb_gpu as PB  # noqa: E402
import textcraft as tc  # noqa: E402
from conn_lines_ref import splice  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, AGENT, REPORTER, LAYER = G.NAMES, G.AGENT, NG.REPORTER, KG.LAYER
# the subnet list of the transform network tests behind two categories that hold battery addresses: the v4-mapped ones and the base record, and
# the IPv6 patterns whose first four groups are zero
LABELS = [("ten", ["10.0.0.0/8"]), ("low half", ["::/64"])] + NG.CATEGORIES
RULES = {"flags on": dict(NG.ALL, labels=LABELS), "flags off": dict(NG.ALL, labels=LABELS, flags=False)}
EXACT = 1 << 53
ROUTES = (["plain", "content", "netev"] + ["tls %d" % p for p in (0, 1, 2)] + ["k8s %d" % p for p in (0, 1, 2)] +
          ["net %d flags %s" % (p, f) for p in (0, 1, 2) for f in ("on", "off")] + ["conn %d" % p for p in (0, 1, 2)] + ["conn_json"])


class World:
    """The handle and the caller tables every route shares."""


@pytest.fixture(scope="module")
def world(nf):
    w = World()
    dt = (nf.FLOW_RECORD, nf.ROLLUP_KINDS)
    w.dt, w.battery = dt, tc.battery(*dt)
    w.entries = KG.entries_for(w.battery.recs, every=16)
    with nf.FlowTable(max_entries=64) as tab, tab.tls_names() as tls, tab.netev_table(E.ANSWERS.items()) as ne, tab.k8s_table(w.entries, LAYER) as k8s, \
            NC.net_table(nf, RULES["flags on"], tab) as net_on, NC.net_table(nf, RULES["flags off"], tab) as net_off:
        w.tab, w.tls, w.tls_ref, w.ne, w.k8s, w.net = tab, tls, T.table_of(nf.GO_TLS_NAMES), ne, k8s, {"on": net_on, "off": net_off}
        w.names = G.table(nf, NAMES)
        yield w


def test_the_battery_meets_the_tables(nf, world):
    """The TLS ids of the battery have no name in the Go table; the Kubernetes table and the subnet list hold battery addresses on both sides."""
    for v in tc.TLS_FALLBACK_IDS:
        assert (T.VERSION, v) not in world.tls_ref
    assert sum((T.CIPHER_SUITE, v) not in world.tls_ref for v in tc.TLS_FALLBACK_IDS) >= 4
    assert all((T.GROUP, v) not in world.tls_ref for v in tc.EDGES[5])
    b = tc.take(world.battery, np.flatnonzero(world.battery.family == "addr"))
    want = RN.encode(b.recs, world.tls_ref, K.table_of(world.entries), LAYER, RULES["flags on"], tc.now_of(tc.CLOCKS[0]), tc.CLOCKS[0][2], G.rows(NAMES), REPORTER, 0)[0]
    for text in (b'"SrcK8S_Name":"obj-', b'"DstK8S_Name":"obj-', b'"SrcSubnetLabel":"', b'"DstSubnetLabel":"', b'"DstSubnetLabel":"high v6"', b'"SrcSubnetLabel":"ten"',
                 b'"DstSubnetLabel":"ten"', b'"SrcSubnetLabel":"low half"', b'"DstSubnetLabel":"low half"'):
        assert text in want, text
    assert 20 <= len(world.entries) <= 80


def test_coverage_report(nf, O, world, capsys):
    old, new = tc.coverage(G.stream(nf, O, 50_000, seed=50_001)), tc.coverage(world.battery.recs)
    with capsys.disabled():
        print("\nvalue shapes reached: seeded stream n = 50 000: %r; battery n = %d: %r" % (old, len(world.battery.recs), new))
    assert new["patterns"] == 256 and new["ties"] == 26 and new["edges"] == new["edges_of"]


# ---- a battery as the inputs of a policy
def netev_part(nf, b):
    """The network-events part of test_netev_gpu.crafted over a battery: its cookie patterns by index, the bit on seven flows of eight."""
    n = len(b.recs)
    ne = np.zeros(n, dtype=nf.NETWORK_EVENTS)
    for i in range(n):
        c, pk, by = E.PATTERNS[i % len(E.PATTERNS)]
        ne["network_events"][i] = np.frombuffer(b"".join(c), dtype=np.uint8).reshape(4, 8)
        ne["packets"][i], ne["bytes"][i] = pk, by
    present = b.present.copy()
    present[np.arange(n) % 8 != 7] |= np.uint8(N.FEAT_NETEV)
    return present, dict(b.parts, network_events=ne)


def policy_inputs(nf, b, policy):
    """(present, parts, answers) of policy 0 (records only), 1 (the feature parts), 2 (network events as well)."""
    if policy == 0:
        return None, None, None
    if policy == 1:
        return b.present, b.parts, None
    return netev_part(nf, b) + (E.ANSWERS,)


def resolved(present, parts, answers):
    """(present, parts, events, resolve result) as the restatements take them."""
    if answers is None:
        return present, parts, None, None
    res = N.resolve(present, parts["network_events"], parts["drops"], answers)
    return res[0], dict(parts, drops=res[1]), res[3], res


def plain_both(nf, w, recs, now, mono, received):
    """nfagg_encode_flp_json, host and device: the size query, one byte short (nothing written), the write with canaries behind it."""
    import torch
    tab, n = w.tab, len(recs)
    host = tab.encode_flp_json(recs, now, mono, w.names, AGENT, received)
    need = len(host[0])
    o, keep = nf.flp_options(now, mono, w.names, AGENT, received)
    small, off, flags = np.full(need - 1, 0xAB, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.full(n, 0xCD, dtype=np.uint8)
    got, n_def = C.c_size_t(0), C.c_size_t(0)
    rc = nf._lib.lib.nfagg_encode_flp_json(tab._h, recs.ctypes.data_as(C.c_void_p), n, C.byref(o), small.ctypes.data_as(C.c_void_p), len(small),
                                           off.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p), C.byref(n_def), C.byref(got))
    assert rc == nf.TRUNCATED and got.value == need and (small == 0xAB).all() and not off.any() and (flags == 0xCD).all()
    d_recs = E.dev(recs)
    d_out = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_def = torch.full((n,), 0xCD, dtype=torch.uint8, device="cuda")
    args = (d_recs.data_ptr(), n, now, mono, w.names, AGENT, received)
    rc, size, nd = tab.encode_flp_json_device(*args, 0, 0, d_off.data_ptr())
    assert rc == nf.TRUNCATED and size == need
    rc, size, nd = tab.encode_flp_json_device(*args, d_out.data_ptr(), need - 1, d_off.data_ptr(), d_def.data_ptr())
    torch.cuda.synchronize()
    assert rc == nf.TRUNCATED and size == need and bool((d_out == 0xAB).all()) and bool((d_def == 0xCD).all())
    rc, wrote, nd = tab.encode_flp_json_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), d_def.data_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert rc == nf.OK and wrote == need and nd == 0 and (out[need:] == 0xAB).all()
    return host, (out[:need], d_off.cpu().numpy(), d_def.cpu().numpy())


def netev_both(nf, w, recs, present, parts, rows, now, mono, received):
    """nfagg_encode_flp_json_netev, host and device, with the protocol of test_netev_gpu.device_encode_json plus the short buffer."""
    import torch
    tab, n = w.tab, len(recs)
    host = tab.encode_flp_json_netev(recs, present, parts, rows, w.ne, now, mono, w.names, AGENT, received)
    d_recs, d_present, d_rows = E.dev(recs), E.dev(present), E.dev(rows)
    d_parts = {k: E.dev(v) for k, v in parts.items() if k != "network_events"}
    args = (d_recs.data_ptr(), n, d_present.data_ptr(), {k: v.data_ptr() for k, v in d_parts.items()}, d_rows.data_ptr(), w.ne, now, mono, w.names, AGENT, received)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_def = torch.full((n,), 0xCD, dtype=torch.uint8, device="cuda")
    rc, need, _ = tab.encode_flp_json_netev_device(*args, 0, 0, d_off.data_ptr())
    assert rc == nf.TRUNCATED and need == len(host[0])
    d_out = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    rc, short, _ = tab.encode_flp_json_netev_device(*args, d_out.data_ptr(), need - 1, d_off.data_ptr(), d_def.data_ptr())
    torch.cuda.synchronize()
    assert rc == nf.TRUNCATED and short == need and bool((d_out == 0xAB).all())
    rc, wrote, n_def = tab.encode_flp_json_netev_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), d_def.data_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert rc == nf.OK and wrote == need and n_def == 0 and (out[need:] == 0xAB).all()
    return host, (out[:need], d_off.cpu().numpy(), d_def.cpu().numpy())


def conversations(b, now, mono):
    """One conversation per battery record: its addresses, ports, protocol and id as the keys, its MACs, ethertype, dscp, directions and
    the two flow times (the restatement's milliseconds) as the first snapshot, the same with the endpoints swapped as the last."""
    i, m = b.recs["id"], b.recs["metrics"]
    specs = []
    for k in range(len(b.recs)):
        src, dst = (R.go_ip(i[f][k].tobytes()).decode() for f in ("src_ip", "dst_ip"))
        assert K.ip16(src) == i["src_ip"][k].tobytes() and K.ip16(dst) == i["dst_ip"][k].tobytes()
        sport, dport, proto = int(i["src_port"][k]), int(i["dst_port"][k]), int(i["transport_protocol"][k])
        start, end = (R.unix_milli(now, mono, int(m[f][k])) for f in ("start_mono_time_ts", "end_mono_time_ts"))
        dirs = [int(m["direction_first_seen"][k])] + [int(x) for x in m["observed_direction"][k][:min(int(m["nb_observed_intf"][k]), 6)]]
        first = CC.snap(src, dst, sport, dport, proto, m["src_mac"][k].tobytes(), m["dst_mac"][k].tobytes(), int(m["eth_protocol"][k]), int(m["dscp"][k]), start, end, dirs)
        last = CC.snap(dst, src, dport, sport, proto, m["dst_mac"][k].tobytes(), m["src_mac"][k].tobytes(), int(m["eth_protocol"][k]), int(m["dscp"][k]), end, start, dirs[::-1])
        exact = lambda v: max(-(EXACT - 8), min(EXACT - 8, v))  # noqa: E731     the aggregates are float64 in Go: a sum of 2^53 or more defers the line
        specs.append(CC.conv(src, dst, sport, dport, proto, int(b.ids[k]), ("newConnection", "endConnection", "heartbeat")[k % 3], k % 2 == 0,
                             (1 + k % 3, k % 2), (exact(int(m["bytes"][k])), k % 5), (int(m["packets"][k]), 0), exact(start), exact(end), first, last))
    return specs


def run_route(nf, w, route, b, clock):
    now, mono, received = tc.now_of(clock), clock[2], clock[3]
    kind, _, rest = route.partition(" ")
    if kind == "plain":
        recs = tc.without_tls(b.recs)
        want = R.encode(recs, now, mono, G.rows(NAMES), AGENT, received)
        for got in plain_both(nf, w, recs, now, mono, received):
            G.check(got, want)
        return want[0]
    if kind == "content":
        recs = tc.without_tls(b.recs)
        want = RC.encode(recs, b.present, b.parts, now, mono, G.rows(NAMES), AGENT, received)
        G.check(w.tab.encode_flp_json_content(recs, b.present, b.parts, now, mono, w.names, AGENT, received), want)
        G.check(CG.device_encode(nf, w.tab, recs, b.present, b.parts, w.names, AGENT, received, now=now, mono=mono), want)
        return want[0]
    if kind == "netev":
        recs = tc.without_tls(b.recs)
        present, parts = netev_part(nf, b)
        rp, rparts, events, res = resolved(present, parts, E.ANSWERS)
        dparts = dict({k: v for k, v in parts.items() if k != "network_events"}, drops=res[1].copy().view(nf.PKT_DROP).reshape(-1))
        want = N.encode_json(recs, rp, dparts, events, now, mono, G.rows(NAMES), AGENT, received)
        for got in netev_both(nf, w, recs, rp, dparts, res[2], now, mono, received):
            G.check(got, want)
        return want[0]
    if kind == "conn_json":
        return CL.check_conv(nf, w.tab, CC.FIELDS_32, conversations(b, now, mono), entries=w.entries, layer=LAYER, rules=RULES["flags on"])[0]
    policy = int(rest.split()[0])
    present, parts, answers = policy_inputs(nf, b, policy)
    rp, rparts, events, res = resolved(present, parts, answers)
    ne = w.ne if answers is not None else None
    kw = dict(received=received, now=now, mono=mono)
    if kind == "tls":
        want = T.encode(b.recs, w.tls_ref, now, mono, G.rows(NAMES), AGENT, received, present=rp, parts=rparts, events=events)
        gots = TG.both_entry_points(nf, w.tab, w.tls, b.recs, present, parts, ne, res, names=w.names, agent=AGENT, **kw)
    elif kind == "k8s":
        want = K.encode(b.recs, w.tls_ref, K.table_of(w.entries), LAYER, now, mono, G.rows(NAMES), REPORTER, received, present=rp, parts=rparts, events=events)
        gots = KG.both_entry_points(nf, w.tab, w.tls, w.k8s, b.recs, present, parts, ne, res, names=w.names, agent=REPORTER, **kw)
    else:
        flags = rest.split()[-1] if kind == "net" else "on"
        want = RN.encode(b.recs, w.tls_ref, K.table_of(w.entries), LAYER, RULES["flags " + flags], now, mono, G.rows(NAMES), REPORTER, received, present=rp,
                         parts=rparts, events=events)
        if kind == "net":
            gots = NG.both_entry_points(nf, w.tab, w.tls, w.k8s, w.net[flags], b.recs, present, parts, ne, res, names=w.names, agent=REPORTER, **kw)
        else:
            want = splice(want, b.recs, b.ids)
            gots = CL.both_entry_points(nf, w.tab, w.tls, w.k8s, w.net[flags], b.recs, b.ids, present, parts, ne, res, names=w.names, agent=REPORTER, **kw)
    for got in gots:
        KG.check(got, want)                                   # reports the first line that differs
    return want[0]


def other_clock_battery(w, clock):
    """The clocks family of a call with half of the digits family, interleaved: a wave and a half under each of the other clocks."""
    digits = tc.family(*w.dt, "digits", clock)
    b = tc.concat([tc.family(*w.dt, "clocks", clock), tc.take(digits, np.arange(0, len(digits.recs), 2)), tc.family(*w.dt, "hash_id", clock)])
    return tc.arrange(b, "interleaved", *w.dt, clock)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("arrangement", tc.ARRANGEMENTS)
def test_battery_through_every_line_kernel_pair(nf, world, arrangement, route):
    b = tc.arrange(world.battery, arrangement, *world.dt)
    assert len(b.recs) <= 4000
    text = run_route(nf, world, route, b, tc.CLOCKS[0])
    whole = arrangement != "odd lane"                         # the odd lanes hold a choice of the battery
    if route != "conn_json" and whole:
        assert b'"SrcAddr":"::"' in text and b'"DstAddr":"::"' in text
        assert route.startswith("conn") or b'"Bytes":18446744073709551615,' in text and b'"Bytes":1000000000000000001,' in text   # conntrack drops ICMP flows
    if route.startswith("net") and route.endswith("on"):
        assert b'"Flags":["' in text and b'"Flags":9' not in text
    if route.startswith("net") and route.endswith("off"):
        assert b'"Flags":["' not in text and (b'"Flags":10000,' in text or not whole)
    if route.startswith("conn ") and whole:
        assert b'"_HashId":"ffffffffffffffff"' in text and b'"_HashId":"100000000"' in text
    if arrangement == "interleaved":                          # the other calls: their clocks family, TimeReceived at its edges
        for clock in tc.CLOCKS[1:]:
            text = run_route(nf, world, route, other_clock_battery(world, clock), clock)
            if route != "conn_json":
                assert b'"TimeReceived":%d,' % clock[3] in text


# ---- protobuf and IPFIX: the clocks and digits families under every clock
def export_battery(w, clock):
    return tc.concat([tc.family(*w.dt, "clocks", clock), tc.family(*w.dt, "digits", clock)])


@pytest.mark.parametrize("call", range(len(tc.CLOCKS)))
def test_clocks_and_digits_through_protobuf(nf, O, world, call):
    clock = tc.CLOCKS[call]
    now, mono = tc.now_of(clock), clock[2]
    b = export_battery(world, clock)
    m = b.recs["metrics"]
    for bits, field in ((64, m["bytes"]), (32, m["packets"]), (16, b.recs["id"]["src_port"])):      # every varint length of the field's type
        have = set(field.tolist())
        assert all(v in have for k in range(1, 10) for v in (2**(7 * k) - 1, 2**(7 * k)) if v < 2**bits)
    contents = XE.oracle_contents(nf, O, b.recs, b.present, b.parts)
    p_present, p_parts = PB._split_contents(nf, O, contents)
    assert np.array_equal(p_present, b.present)
    orecs = b.recs.view(O.FLOW_RECORD)
    agent = [PB.AGENT4, XE.AGENT6][call % 2]
    opts = O.pb_options(now, mono, agent, O.intf_table(PB.NAMES))
    buf, off, blen, keys = world.tab.encode_pb(b.recs, now, mono, agent, nf.intf_table(PB.NAMES), kafka_keys=True)
    assert PB.frames(buf, off, blen) == O.pb_encode(orecs, opts)
    assert int(off[0]) == 0 and int(off[-1]) == len(buf) and np.array_equal(keys, O.kafka_keys(orecs))
    buf, off, blen = world.tab.encode_pb(PB._records_of(nf, O, orecs["id"], contents), now, mono, agent, nf.intf_table(PB.NAMES), present=p_present, parts=p_parts)
    assert PB.frames(buf, off, blen) == O.pb_encode_contents(orecs["id"], contents, opts)
    assert int(off[0]) == 0 and int(off[-1]) == len(buf)


@pytest.mark.parametrize("call", range(len(tc.CLOCKS)))
def test_clocks_and_digits_through_ipfix(nf, world, call):
    clock = tc.CLOCKS[call]
    now, mono = tc.now_of(clock), clock[2]
    b = export_battery(world, clock)
    rows = [(i, m, name.encode()) for (i, m, name, _) in PB.NAMES]
    want, want_off = IR.encode(b.recs, now, mono, rows, XE.EXPORT, 0xFFFFFF00 + call)
    buf, off = world.tab.encode_ipfix(b.recs, now, mono, nf.intf_table(PB.NAMES), XE.EXPORT, 0xFFFFFF00 + call)
    assert off.tolist() == want_off.tolist()
    if buf.tobytes() != want:
        k = next(i for i in range(len(b.recs)) if buf.tobytes()[int(off[i]):int(off[i + 1])] != want[int(off[i]):int(off[i + 1])])
        raise AssertionError("message %d (%s):\n got %s\nwant %s" % (k, b.family[k], buf.tobytes()[int(off[k]):int(off[k + 1])].hex(), want[int(off[k]):int(off[k + 1])].hex()))
