"""`extract timebased` on the GPU (nfagg_timebased_*, csrc/nfagg_timebased.hip) through the C ABI, the host-memory and the
device entry points side by side, against the flow-by-flow restatement of tests/timebased_ref.py: sizes around a wave and a
workgroup, 2^17 + 1 keys, one hot key and all-distinct keys, keys crafted onto one home slot / past the table's end / onto one
first key word, every served column and the widest key, the presence rules, a sequence of windows with boundary stamps, dead and
returning keys, all seven operations under every topK shape, ties across the K-th place, large values and the inexact flag, the
deferral, the overflow, a results buffer that is too small, and the stage end to end.

How results are compared (the reference's tie order is Go's map order, so it is unspecified): for topK == 0 as {key text:
value}; for topK > 0 the lengths are equal, the sequences of values are equal element by element, the keys are distinct, and every
reported key's value is the restatement's full result for that key. Values compare with == on float64 and on their bytes; no
tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_content_ref as C  # noqa: E402
import flp_json_k8s_ref as K  # noqa: E402
import flp_json_net_ref as R  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_flp_json_k8s_gpu as KG  # noqa: E402
import test_flp_json_net_cpu as NC  # noqa: E402
import test_flp_json_net_gpu as NG  # noqa: E402
import timebased_ref as T  # noqa: E402
from flp_json_ref import record_to_map  # noqa: E402

pytestmark = pytest.mark.gpu

S = 10**9
NAMES, NOW, MONO, RECEIVED = G.NAMES, G.NOW, G.MONO, G.RECEIVED
LAYER, REPORTER, ALL = KG.LAYER, NG.REPORTER, NG.ALL
OPS = ("sum", "avg", "min", "max", "count", "last", "diff")
V4 = bytes(10) + b"\xff\xff"


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()                 # the upload runs on torch's stream, the library's calls on its own
    return t


# ---- flows
def addrs_v4(ids):
    """10.x.y.z of the integers ids (below 2^24), as n x 16 bytes."""
    ids = np.asarray(ids, dtype=np.int64)
    a = np.zeros((len(ids), 16), dtype=np.uint8)
    a[:, 10:12], a[:, 12], a[:, 13], a[:, 14], a[:, 15] = 0xFF, 10, (ids >> 16) & 255, (ids >> 8) & 255, ids & 255
    return a


def make_recs(nf, src, dst=None, nbytes=1, packets=1, proto=6, sport=1000, dport=443, eth=0x0800):
    n = len(src)
    r = np.zeros(n, dtype=nf.FLOW_RECORD)
    r["id"]["src_ip"] = src
    r["id"]["dst_ip"] = dst if dst is not None else addrs_v4(np.zeros(n, dtype=np.int64) + 0xABCDEF)
    r["id"]["src_port"], r["id"]["dst_port"], r["id"]["transport_protocol"] = sport, dport, proto
    r["metrics"]["eth_protocol"], r["metrics"]["bytes"], r["metrics"]["packets"] = eth, nbytes, packets
    return r


def plain_maps(nf, recs, present=None, parts=None):
    """RecordToMap of the keys the stage reads, with its presence rules (decode_protobuf.go:87-116, record.go:116-125): what
    tests/flp_json_ref.record_to_map writes for them (test_plain_maps_are_record_to_map checks that), fast enough for 2^17 flows."""
    go_ip = nf.filter.go_ip_string
    memo = {}

    def ip(b):
        b = b.tobytes()
        if b not in memo:
            memo[b] = go_ip(b)
        return memo[b]
    out = []
    k, m = recs["id"], recs["metrics"]
    for i in range(len(recs)):
        d = {}
        if int(m["bytes"][i]):
            d[b"Bytes"] = int(m["bytes"][i])
        if int(m["packets"][i]):
            d[b"Packets"] = int(m["packets"][i])
        proto = int(k["transport_protocol"][i])
        if int(m["eth_protocol"][i]) in (0x0800, 0x86DD):
            d[b"SrcAddr"], d[b"DstAddr"], d[b"Proto"] = ip(k["src_ip"][i]), ip(k["dst_ip"][i]), proto
            if proto in (6, 17, 132):
                d[b"SrcPort"], d[b"DstPort"] = int(k["src_port"][i]), int(k["dst_port"][i])
        if present is not None and int(present[i]) & 1 and int(parts["additional"]["flow_rtt"][i]):
            v = int(parts["additional"]["flow_rtt"][i])
            d[b"TimeFlowRttNs"] = v - 2**64 if v >> 63 else v
        out.append(d)
    return out


def rule(name, keys, op, opkey="Bytes", top=0, rev=False, interval=60 * S):
    return dict(name=name, indexKeys=list(keys), operationType=op, operationKey=opkey, topK=top, reversed=rev, timeInterval=interval)


def specs_of(nf, rules):
    from netobserv_ebpf_agent_amd.timebased import OPERATIONS
    return [dict(index_keys=r["indexKeys"], operation=OPERATIONS[r["operationType"]], value=nf.metrics.VALUE_SOURCES[r["operationKey"]], top_k=r["topK"],
                 reversed=r["reversed"], interval_ns=r["timeInterval"]) for r in rules]


# ---- the two entry points against the restatement
def key_texts(nf, tb, r, rules, ids):
    from netobserv_ebpf_agent_amd.timebased import render_column
    t = tb.table_of_rule[r]
    keys = tb.keys(t, ids)
    return [",".join(render_column(k, keys[j]["col"][c], tb, t, c) for c, k in enumerate(rules[r]["indexKeys"])) for j in range(len(ids))]


def check_rule(nf, tb, r, rules, res, ref, flags_zero=True):
    f = ref.filters[r]
    full = f["results"]
    texts = key_texts(nf, tb, r, rules, res["key"])
    values = [float(v) for v in res["value"]]
    assert len(set(texts)) == len(texts), "rule %d: a key twice" % r
    if flags_zero:
        assert not res["flags"].any(), "rule %d: flags" % r
    k = rules[r]["topK"]
    if k == 0:
        assert set(texts) == set(full), "rule %d: keys" % r
        for t, v in zip(texts, values):
            assert T.same_bits(v, full[t]), (r, t, v, full[t])
        return
    want = [v for _, v in f["output"]]
    assert len(values) == len(want) == min(k, len(full)), "rule %d: %d results, the restatement has %d" % (r, len(values), len(want))
    for j, (a, b) in enumerate(zip(values, want)):
        assert T.same_bits(a, b), "rule %d, place %d: %r, the restatement has %r" % (r, j, a, b)
    for t, v in zip(texts, values):
        assert t in full and T.same_bits(v, full[t]), (r, t, v, full.get(t))


def device_extract(nf, tab, tb, recs, now, k8s_rows, net_rows, features, caps):
    """nfagg_timebased_extract_device into buffers of exactly the caps with 0xAB canaries over them and 128 bytes behind."""
    import torch
    n = len(recs)
    d_recs = dev(recs) if n else None
    d_k = dev(np.ascontiguousarray(k8s_rows, dtype=np.uint32)) if k8s_rows is not None and n else None
    d_n = dev(net_rows) if net_rows is not None and n else None
    d_feats, keep = None, {}
    if features is not None and n:
        keep = {k: dev(v) for k, v in features[1].items() if k in ("additional", "dns", "drops") and v is not None}
        d_present = dev(np.ascontiguousarray(features[0], dtype=np.uint8))
        d_feats = (d_present.data_ptr(), {k: v.data_ptr() for k, v in keep.items()})
    d_outs = [torch.full((c * 16 + 128,), 0xAB, dtype=torch.uint8, device="cuda") for c in caps]
    torch.cuda.synchronize()
    rc, counts, missing = tab.timebased_extract_device(tb, d_recs.data_ptr() if n else 0, n, now, d_k.data_ptr() if d_k is not None else 0,
                                                       d_n.data_ptr() if d_n is not None else 0, caps, [o.data_ptr() for o in d_outs], d_feats)
    torch.cuda.synchronize()
    outs = []
    for o, c in zip(d_outs, counts):
        raw = o.cpu().numpy()
        used = c * 16 if rc == nf.OK else 0
        assert (raw[used:] == 0xAB).all(), "bytes behind the results were written"
        outs.append(raw[:used].copy().view(nf.TB_RESULT))
    return rc, outs, counts, missing


class Pair:
    """One rule set twice on the device, one object fed through the host-memory entry point and one through the device entry
    point, and the restatement; call() feeds all three and compares."""

    def __init__(self, nf, tab, rules, k8s=None, net=None, max_keys=1 << 12):
        self.nf, self.tab, self.rules = nf, tab, rules
        self.ref = T.Timebased(rules)
        self.tbs = [tab.timebased_rules(specs_of(nf, rules), k8s, net, max_keys) for _ in range(2)]

    def close(self):
        for tb in self.tbs:
            tb.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def call(self, recs, maps, now, k8s_rows=None, net_rows=None, features=None, caps=None, flags_zero=True, check=True):
        nf = self.nf
        self.ref.extract(maps, now)
        caps = caps or [max(r["topK"], self.tbs[0].max_keys) if r["topK"] == 0 else r["topK"] for r in self.rules]
        rc, res, counts, missing = self.tab.timebased_extract(self.tbs[0], recs, now, k8s_rows, net_rows, features, caps)
        rc_d, res_d, counts_d, missing_d = device_extract(nf, self.tab, self.tbs[1], recs, now, k8s_rows, net_rows, features, caps)
        assert (rc, counts, missing) == (rc_d, counts_d, missing_d) and rc == nf.OK and missing == 0
        if check:
            for r in range(len(self.rules)):
                assert counts[r] == len(res[r]) == len(res_d[r])
                check_rule(nf, self.tbs[0], r, self.rules, res[r], self.ref, flags_zero)
                check_rule(nf, self.tbs[1], r, self.rules, res_d[r], self.ref, flags_zero)
        return res, res_d


def test_plain_maps_are_record_to_map(nf):
    rng = np.random.default_rng(2)
    n = 64
    recs = make_recs(nf, addrs_v4(rng.integers(0, 9, n)), addrs_v4(rng.integers(0, 9, n)), rng.integers(0, 3, n), rng.integers(0, 3, n),
                     rng.choice([1, 6, 17, 58, 132, 47], n), rng.integers(0, 65536, n), rng.integers(0, 65536, n), rng.choice([0x0800, 0x86DD, 0x0806], n))
    recs["id"]["src_ip"][::5] = np.frombuffer(bytes.fromhex("20010db8000000000000000000000001"), dtype=np.uint8)
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 144)
    names, memo = G.rows(NAMES), {}
    for i, mine in enumerate(plain_maps(nf, recs)):
        full = record_to_map(raw[i].tobytes(), NOW, MONO, names, REPORTER, RECEIVED, b"unknown", memo)
        assert mine == {k: v for k, v in full.items() if k in (b"SrcAddr", b"DstAddr", b"SrcPort", b"DstPort", b"Proto", b"Bytes", b"Packets")}, i


# ---- 1. sizes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_sizes(nf, tab, n):
    rng = np.random.default_rng(n)
    rules = [rule("bytes", ["SrcAddr"], "sum"), rule("conv", ["SrcAddr", "DstAddr", "SrcPort", "DstPort"], "count", top=5),
             rule("proto", ["Proto"], "max", "Packets", top=3, rev=True), rule("diff", ["SrcAddr"], "diff", "Packets", top=4)]
    recs = make_recs(nf, addrs_v4(rng.integers(0, 40, n)), addrs_v4(rng.integers(0, 5, n)), rng.integers(1, 10**6, n), rng.integers(1, 100, n),
                     rng.choice([6, 17, 132], n), rng.integers(1, 4, n), rng.integers(1, 4, n))
    with Pair(nf, tab, rules) as p:
        p.call(recs, plain_maps(nf, recs), 100 * S)
        p.call(recs[::-1], plain_maps(nf, recs[::-1]), 101 * S)              # the keys are there already: no new id
        st = p.tbs[0].stats()
        assert st.keys[0] == len(np.unique(recs["id"]["src_ip"], axis=0)) and st.slices[0] == (2 if n else 0) and st.bytes_held > 0


def test_2_17_plus_1_flows_on_as_many_addresses(nf, tab):
    n = (1 << 17) + 1
    rng = np.random.default_rng(17)
    recs = make_recs(nf, addrs_v4(rng.permutation(1 << 20)[:n]), nbytes=1000 + rng.permutation(n), packets=7)
    rules = [rule("top", ["SrcAddr"], "sum", top=10), rule("bot", ["SrcAddr"], "sum", top=4096, rev=True), rule("all", ["SrcAddr"], "avg")]
    with Pair(nf, tab, rules, max_keys=n) as p:                            # a cap of exactly the keys
        res, res_d = p.call(recs, plain_maps(nf, recs), 5 * S, check=False)
        assert p.tbs[0].stats().keys[0] == n == len(res[2]) == len(res_d[2]) and p.tbs[0].stats().slots[0] == 1 << 19
        for r in range(3):
            check_rule(nf, p.tbs[0], r, rules, res[r], p.ref)
        for r in range(2):
            check_rule(nf, p.tbs[1], r, rules, res_d[r], p.ref)
        assert np.array_equal(np.sort(res[2]["value"]), np.sort(res_d[2]["value"])) and len(np.unique(res_d[2]["key"])) == n and not res_d[2]["flags"].any()
        # every value is distinct: the order is pinned, and both entry points report the same flows in it
        for r in (0, 1):
            assert key_texts(nf, p.tbs[0], r, rules, res[r]["key"]) == key_texts(nf, p.tbs[1], r, rules, res_d[r]["key"])
        assert res[0]["value"][0] == 1000.0 + n - 1 and res[1]["value"][0] == 1000.0


# ---- 2. contention and crafted placement
def test_all_flows_on_one_key_and_every_flow_its_own(nf, tab):
    n = 4097
    rules = [rule(op, ["SrcAddr"], op, top=0 if k % 2 else 3) for k, op in enumerate(OPS)]
    rng = np.random.default_rng(1)
    hot = make_recs(nf, addrs_v4(np.zeros(n, dtype=np.int64) + 77), nbytes=rng.integers(1, 2**40, n))
    own = make_recs(nf, addrs_v4(np.arange(n)), nbytes=rng.integers(1, 2**40, n))
    with Pair(nf, tab, rules, max_keys=n) as p:
        p.call(hot, plain_maps(nf, hot), 1 * S)
        assert p.tbs[0].stats().keys[0] == 1
        p.call(own, plain_maps(nf, own), 2 * S)
        assert p.tbs[0].stats().keys[0] == n                                # 10.0.0.77 is one of them
        p.call(hot[:100], plain_maps(nf, hot[:100]), 3 * S)


def crafted_addresses(nf, tb, slots):
    """Addresses searched on the CPU against the table's hash, as tests/conncraft.py searches its keys: v4-mapped ones (one first
    key word: the eight leading zero bytes; they differ in the second and third) and IPv6 ones, grouped by home slot."""
    cand = np.zeros(60_000, dtype=nf.TB_KEY)
    a = addrs_v4(np.arange(40_000) * 37 + 5)
    cand["col"][:40_000, 0] = a
    v6 = np.zeros((20_000, 16), dtype=np.uint8)
    v6[:, 0], v6[:, 1], v6[:, 6], v6[:, 7], v6[:, 15] = 0x20, 0x01, np.arange(20_000) >> 8, np.arange(20_000) & 255, 1
    cand["col"][40_000:, 0] = v6
    home = tb.key_hash(0, cand) & np.uint64(slots - 1)
    return cand["col"][:, 0], home.astype(np.int64)


def test_crafted_placement(nf, tab):
    """A table of the minimum size (1 024 slots). Twenty v4-mapped keys on one home slot: they share their first key word and
    differ in a later one, so a probe meets slots whose first word matches and whose second does not. Twelve keys (both families)
    on the last slot: the chain runs past the table's end. Sixteen on slot 1 022, whose chain meets that one. max_keys is exactly
    their number."""
    rules = [rule("sum", ["SrcAddr"], "sum"), rule("last", ["SrcAddr"], "last", "Packets"), rule("top", ["SrcAddr"], "count", top=7)]
    with tab.timebased_rules(specs_of(nf, rules), None, None, 48) as probe:
        slots = probe.stats().slots[0]
        assert slots == 1024
        addr, home = crafted_addresses(nf, probe, slots)
    v4 = np.arange(len(addr)) < 40_000
    count = np.bincount(home[v4], minlength=slots)
    busy = int(np.argmax(np.where(np.arange(slots) < 1000, count, 0)))
    pick = np.concatenate([np.flatnonzero(v4 & (home == busy))[:20], np.flatnonzero(v4 & (home == slots - 1))[:6], np.flatnonzero(~v4 & (home == slots - 1))[:6],
                           np.flatnonzero(home == slots - 2)[:16]])
    assert len(pick) == 48 and (~v4[pick]).any() and v4[pick].sum() >= 20
    reps = 37
    rng = np.random.default_rng(9)
    order = rng.permutation(np.tile(pick, reps))
    recs = make_recs(nf, addr[order], nbytes=rng.integers(1, 10**9, len(order)), packets=rng.integers(1, 10**6, len(order)))
    with Pair(nf, tab, rules, max_keys=48) as p:
        res, _ = p.call(recs, plain_maps(nf, recs), 1 * S)
        assert len(res[0]) == 48 and p.tbs[0].stats().keys[0] == 48
        got_home = p.tbs[0].key_hash(0, p.tbs[0].keys(0, res[0]["key"])) & np.uint64(slots - 1)
        assert sorted(np.bincount(got_home.astype(np.int64), minlength=slots)[[busy, slots - 2, slots - 1]].tolist()) == [12, 16, 20]
        p.call(recs[:500], plain_maps(nf, recs[:500]), 2 * S)               # found again where they were claimed


# ---- 3. key shapes and presence
@pytest.fixture(scope="module")
def world(nf, tab):
    """About 300 flows between the informers' addresses and strangers: IPv4 and IPv6, TCP / UDP / SCTP / ICMP / GRE, a tenth with a
    non-IP ethertype; the informer answers of tests/test_flp_json_k8s_gpu.py (rows without a namespace, without a host, with an
    empty zone) and the subnet categories of tests/test_flp_json_net_gpu.py (one with an empty name); per flow the enriched map."""
    rng = np.random.default_rng(23)
    n = 300
    pool = [K.ip16("10.0.%d.%d" % (a, b)) for a in range(4) for b in (1, 7, 130, 200)] + [K.ip16("2001:db8::%x" % k) for k in range(1, 5)] + \
           [K.ip16("9000::%x" % k) for k in range(1, 3)]
    pick = lambda: np.frombuffer(b"".join(pool[k] for k in rng.integers(0, len(pool), n)), dtype=np.uint8).reshape(n, 16)  # noqa: E731
    src, dst = pick(), pick()
    recs = make_recs(nf, src, dst, rng.integers(1, 10**6, n), rng.integers(1, 100, n), rng.choice([6, 17, 132, 1, 58, 47], n), rng.integers(1, 5, n),
                     rng.integers(1, 5, n), 0x86DD)
    is4 = (src[:, :12] == np.frombuffer(V4, dtype=np.uint8)).all(axis=1)
    recs["metrics"]["eth_protocol"] = np.where(rng.integers(0, 10, n) == 0, 0x0806, np.where(is4, 0x0800, 0x86DD))
    recs["metrics"]["direction_first_seen"] = rng.integers(0, 2, n)
    entries = KG.entries_for(recs)
    table, cats, names = K.table_of(entries), R.parse_subnets(NG.CATEGORIES), G.rows(NAMES)
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 144)
    memo = {}
    maps = [R.apply_rules(record_to_map(raw[i].tobytes(), NOW, MONO, names, REPORTER, RECEIVED, b"unknown", memo), table, LAYER, ALL, cats) for i in range(n)]
    return recs, entries, maps


COLUMNS = ["SrcAddr", "DstAddr", "SrcPort", "DstPort", "Proto", "SrcSubnetLabel", "DstSubnetLabel", "FlowDirection"] + \
          ["SrcK8S_" + f for f in ("Namespace", "Name", "Type", "OwnerName", "OwnerType", "NetworkName", "HostIP", "HostName", "Zone")] + \
          ["DstK8S_" + f for f in ("Namespace", "Name", "Type", "OwnerName", "OwnerType", "NetworkName", "HostIP", "HostName", "Zone")]
SHAPES = [COLUMNS[k:k + 4] for k in range(0, len(COLUMNS), 4)]


@pytest.mark.parametrize("cols", SHAPES, ids=["+".join(c) for c in SHAPES])
def test_every_served_column_alone(nf, tab, world, cols):
    recs, entries, maps = world
    rules = [rule("by " + c, [c], "sum") for c in cols] + [rule("top " + c, [c], "count", "Packets", top=3) for c in cols]
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, ALL, tab) as net, Pair(nf, tab, rules, k8s, net) as p:
        k8s_rows = tab.k8s_resolve(k8s, recs)
        net_rows = tab.net_resolve(net, recs, k8s, k8s_rows, REPORTER)
        res, _ = p.call(recs, maps, 1 * S, k8s_rows, net_rows)
        assert all(len(r) >= 1 for r in res[:len(cols)]), [len(r) for r in res]
        p.call(recs[:50], maps[:50], 2 * S, k8s_rows[:50], net_rows[:50])


def test_the_widest_key_and_presence(nf, tab, world):
    recs, entries, maps = world
    rules = [rule("conv", ["SrcAddr", "DstAddr", "SrcPort", "DstPort"], "sum"), rule("addr", ["SrcAddr"], "count"), rule("ports", ["SrcPort", "Proto"], "count"),
             rule("ns", ["SrcK8S_Namespace", "DstK8S_Namespace", "Proto", "FlowDirection"], "count"), rule("ns top", ["SrcK8S_Namespace", "DstK8S_Namespace", "Proto", "FlowDirection"], "max", top=5)]
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, ALL, tab) as net, Pair(nf, tab, rules, k8s, net) as p:
        k8s_rows = tab.k8s_resolve(k8s, recs)
        net_rows = tab.net_resolve(net, recs, k8s, k8s_rows, REPORTER)
        res, _ = p.call(recs, maps, 1 * S, k8s_rows, net_rows)
    is_ip = np.isin(recs["metrics"]["eth_protocol"], (0x0800, 0x86DD))
    ported = is_ip & np.isin(recs["id"]["transport_protocol"], (6, 17, 132))
    assert 0 < is_ip.sum() < len(recs) and 0 < ported.sum() < is_ip.sum()
    # a non-IP ethertype leaves the SrcAddr table, ICMP and GRE the port tables, a row without a namespace the namespace table
    assert res[1]["value"].sum() == is_ip.sum() and res[2]["value"].sum() == ported.sum() and res[0]["value"].sum() == recs["metrics"]["bytes"][ported].sum()
    with_ns = sum(1 for m in maps if m.get(b"SrcK8S_Namespace") and m.get(b"DstK8S_Namespace") and b"FlowDirection" in m and b"Proto" in m)
    assert 0 < with_ns < is_ip.sum() and res[3]["value"].sum() == with_ns


# ---- 4. windows
def test_windows(nf, tab):
    """Two intervals on one table, A = 10 s and B = 4 s, every operation under both, and two selections in which dead keys lead.
    The slice of the first call sits exactly on now - B in the second call and 1 ns beyond it in the third, exactly on now - A in
    the fourth and 1 ns beyond in the fifth: there c goes dead and stays, with the operations' values for no entry. The sixth call
    shares the fifth's stamp; the seventh only moves time and leaves every key dead; in the eighth c returns."""
    A, B = 10 * S, 4 * S
    rules = [rule(op + " A", ["SrcAddr"], op, interval=A) for op in OPS] + [rule(op + " B", ["SrcAddr"], op, interval=B) for op in OPS] + \
            [rule("max rev", ["SrcAddr"], "max", top=3, rev=True, interval=A), rule("min top", ["SrcAddr"], "min", top=2, interval=B)]
    a, b, c, d = 1, 2, 3, 4
    calls = [(100 * S, [(a, 5), (b, 6), (c, 7), (a, 9)]), (104 * S, [(a, 2)]), (104 * S + 1, []), (110 * S, [(b, 8)]), (110 * S + 1, [(d, 1)]),
             (110 * S + 1, [(a, 4), (a, 3)]), (130 * S, []), (131 * S, [(c, 11)]), (136 * S, []), (141 * S + 1, [])]
    with Pair(nf, tab, rules, max_keys=4) as p:
        seen = []
        for now, flows in calls:
            recs = make_recs(nf, addrs_v4([k for k, _ in flows]), nbytes=[v for _, v in flows])
            res, _ = p.call(recs, plain_maps(nf, recs), now)
            seen.append({t: float(v) for t, v in zip(key_texts(nf, p.tbs[0], 0, rules, res[0]["key"]), res[0]["value"])})
        st = p.tbs[0].stats()
        assert st.keys[0] == 4 and st.slices[0] == 0 and st.last_now_ns == 141 * S + 1      # every slice has been trimmed
    # what the restatement said, spelled out for the sum over A
    assert seen[3] == {"10.0.0.1": 16.0, "10.0.0.2": 14.0, "10.0.0.3": 7.0} and seen[4] == {"10.0.0.1": 2.0, "10.0.0.2": 8.0, "10.0.0.3": 0.0, "10.0.0.4": 1.0}
    assert seen[5]["10.0.0.1"] == 9.0 and set(seen[6].values()) == {0.0} and seen[7]["10.0.0.3"] == 11.0 and seen[9]["10.0.0.3"] == 0.0


# ---- 5. operations and selections
@pytest.mark.parametrize("top", [0, 1, 50, 51, 4096])
def test_all_seven_operations(nf, tab, top):
    """Fifty keys, three calls, the second inside and the first outside the window at the third: topK 0, 1, the number of keys,
    one more, and the cap."""
    rng = np.random.default_rng(top)
    rules = [rule(op, ["SrcAddr"], op, top=top, interval=5 * S) for op in OPS] + [rule(op + " rev", ["SrcAddr"], op, "Packets", top=top, rev=True, interval=5 * S) for op in OPS]
    with Pair(nf, tab, rules, max_keys=64) as p:
        for now, n in ((1 * S, 400), (5 * S, 300), (8 * S, 350)):
            recs = make_recs(nf, addrs_v4(rng.integers(0, 50, n)), nbytes=rng.integers(1, 2**44, n), packets=rng.integers(1, 2**31, n))
            p.call(recs, plain_maps(nf, recs), now)
        assert p.tbs[0].stats().keys[0] == 50


def test_ties_across_the_kth_place(nf, tab):
    """600 keys: 5 at 10, 300 at 7, the rest at 1 .. 3. The 100 best are the five and 95 of the 300; the 400 least all of the
    low ones and 105 of the sevens. 5 000 keys that all count 1: 4 096 of one value."""
    vals = np.concatenate([np.full(5, 10), np.full(300, 7), 1 + np.arange(295) % 3])
    rng = np.random.default_rng(4)
    order = rng.permutation(600)
    recs = make_recs(nf, addrs_v4(order), nbytes=vals[order])
    rules = [rule("top", ["SrcAddr"], "sum", top=100), rule("bot", ["SrcAddr"], "sum", top=400, rev=True), rule("one", ["SrcAddr"], "max", top=1),
             rule("edge", ["SrcAddr"], "sum", top=5), rule("edge+1", ["SrcAddr"], "sum", top=6), rule("low", ["SrcAddr"], "sum", top=295, rev=True)]
    with Pair(nf, tab, rules, max_keys=600) as p:
        res, _ = p.call(recs, plain_maps(nf, recs), 1 * S)
        assert res[0]["value"].tolist() == [10.0] * 5 + [7.0] * 95 and (res[1]["value"][-105:] == 7.0).all() and res[5]["value"].max() == 3.0
    many = make_recs(nf, addrs_v4(np.arange(5000)))
    rules = [rule("count", ["SrcAddr"], "count", top=4096), rule("count rev", ["SrcAddr"], "count", top=4096, rev=True)]
    with Pair(nf, tab, rules, max_keys=5000) as p:
        res, _ = p.call(many, plain_maps(nf, many), 1 * S)
        assert len(res[0]) == 4096 and (res[0]["value"] == 1.0).all() and len(np.unique(res[1]["key"])) == 4096


# ---- 6. large values
def large_call(nf, tab, values, ops=OPS):
    rules = [rule(op, ["SrcAddr"], op) for op in ops]
    recs = make_recs(nf, addrs_v4(np.zeros(len(values), dtype=np.int64) + 1), nbytes=np.array(values, dtype=np.uint64))
    out = []
    for variant in (0, 1):
        with tab.timebased_rules(specs_of(nf, rules), None, None, 8) as tb:
            caps = [4] * len(rules)
            if variant == 0:
                rc, res, counts, _ = tab.timebased_extract(tb, recs, 1 * S, None, None, None, caps)
            else:
                rc, res, counts, _ = device_extract(nf, tab, tb, recs, 1 * S, None, None, None, caps)
            assert rc == nf.OK and counts == [1] * len(rules)
            out.append({op: (float(r["value"][0]), int(r["flags"][0])) for op, r in zip(ops, res)})
    assert out[0] == out[1]
    return out[0]


def test_large_values(nf, tab):
    I = nf._lib.TB_INEXACT
    # a sum of exactly 2^53 - 1: exact, and equal to the restatement's float sum in any order
    got = large_call(nf, tab, [2**53 - 2, 1])
    assert got["sum"] == (float(2**53 - 1), 0) and got["avg"] == (float(2**53 - 1) / 2.0, 0) and got["max"] == (float(2**53 - 2), 0)
    assert got["diff"] == (1.0 - float(2**53 - 2), 0) and got["count"] == (2.0, 0) and got["last"] == (1.0, 0) and got["min"] == (1.0, 0)
    ref = T.Timebased([rule("s", ["SrcAddr"], "sum")])
    ref.extract([{"SrcAddr": "k", "Bytes": 2**53 - 2}, {"SrcAddr": "k", "Bytes": 1}], 0)
    assert ref.filters[0]["results"]["k"] == got["sum"][0]
    # a sum that reaches 2^53: the correctly rounded exact total, flagged
    got = large_call(nf, tab, [2**53 - 1, 1])
    assert got["sum"] == (float(2**53), I) and got["avg"] == (float(2**53) / 2.0, I) and got["max"] == (float(2**53 - 1), 0) and got["count"] == (2.0, 0)
    got = large_call(nf, tab, [2**53 + 1])                                  # one value that float64 cannot hold: 2^53, flagged
    assert got["sum"] == (float(2**53), I) and got["min"] == (float(2**53 + 1), 0) and got["last"] == (float(2**53 + 1), 0)
    got = large_call(nf, tab, [2**53, 2**53 + 3])                           # 2^54 + 3 lies between 2^54 and 2^54 + 4, nearer the latter
    assert got["sum"] == (float(2**54 + 3), I) and float(2**54 + 3) == 2.0**54 + 4.0
    # values whose integer sum passes 2^64 (and 2^65): nothing wraps
    big = [2**64 - 1, 2**64 - 1, 2**64 - 1, 5]
    got = large_call(nf, tab, big)
    assert got["sum"] == (float(sum(big)), I) and got["avg"] == (float(sum(big)) / 4.0, I) and sum(big) > 2**65
    assert got["max"] == (float(2**64 - 1), 0) and got["min"] == (5.0, 0) and got["diff"] == (5.0 - float(2**64 - 1), 0) and got["last"] == (5.0, 0)
    # a sticky bit far below the rounding place decides: 2^64 + 2^11 is a tie that rounds to even (down), one more rounds up
    assert large_call(nf, tab, [2**63, 2**63, 2**11], ("sum",))["sum"] == (float(2**64 + 2**11), I) == (2.0**64, I)
    assert large_call(nf, tab, [2**63, 2**63, 2**11, 1], ("sum",))["sum"] == (float(2**64 + 2**11 + 1), I) == (2.0**64 + 4096.0, I)


def test_large_values_across_slices(nf, tab):
    """The 128-bit total is carried across the slices of a window too: three calls of 2^64 - 1 each."""
    rules = [rule("sum", ["SrcAddr"], "sum"), rule("avg", ["SrcAddr"], "avg"), rule("top", ["SrcAddr"], "sum", top=1)]
    with tab.timebased_rules(specs_of(nf, rules), None, None, 8) as tb:
        for k in range(3):
            recs = make_recs(nf, addrs_v4([1, 2]), nbytes=np.array([2**64 - 1, 3], dtype=np.uint64))
            rc, res, counts, _ = tab.timebased_extract(tb, recs, k * S, None, None, None, [4, 4, 1])
        total = 3 * (2**64 - 1)
        assert rc == nf.OK and sorted((float(v), int(f)) for v, f in zip(res[0]["value"], res[0]["flags"])) == [(9.0, 0), (float(total), 1)]
        assert float(res[2]["value"][0]) == float(total)
        assert sorted(res[1]["value"].tolist()) == [3.0, float(total) / 3.0]


def test_a_signed_value_source(nf, tab):
    """TimeFlowRttNs is an int64 in the reference: values are kept with bit 63 flipped. Positive ones behave as Bytes do; a flow
    with the part and an RTT of 0, or without the part, has no TimeFlowRttNs and defers the call."""
    n = 200
    rng = np.random.default_rng(6)
    recs = make_recs(nf, addrs_v4(rng.integers(0, 9, n)))
    present = np.ones(n, dtype=np.uint8)
    parts = dict(additional=np.zeros(n, dtype=nf.ADDITIONAL))
    parts["additional"]["flow_rtt"] = rng.integers(1, 2**40, n)
    rules = [rule(op, ["SrcAddr"], op, "TimeFlowRttNs") for op in OPS] + [rule("bytes", ["SrcAddr"], "sum")]
    with Pair(nf, tab, rules, max_keys=16) as p:
        p.call(recs, plain_maps(nf, recs, present, parts), 1 * S, features=(present, parts))
        present[7], parts["additional"]["flow_rtt"][9] = 0, 0
        rc, _, _, missing = tab.timebased_extract(p.tbs[0], recs, 2 * S, None, None, (present, parts), 64)
        assert (rc, missing) == (nf.EDEFER, 2)
        rc, _, _, missing = tab.timebased_extract(p.tbs[0], recs, 2 * S, None, None, None, 64)         # no features at all: every flow
        assert (rc, missing) == (nf.EDEFER, n)


def content_maps(nf, recs, present, parts):
    """plain_maps plus the keys of the feature parts as tests/flp_json_content_ref.py restates decode_protobuf.go:130-192."""
    return [C.add_content(m, C.flow_parts(present, parts, i)) for i, m in enumerate(plain_maps(nf, recs))]


def test_every_value_source_and_negative_values(nf, tab):
    """DnsLatencyMs (int64 nanoseconds / 10^6 truncating toward zero, present with a DnsId), PktDropBytes and PktDropPackets (present
    with a cause, 0 is a value) and TimeFlowRttNs with negative values, under all seven operations where four sources fit a table.
    min, max, last, diff and count are exact whatever the sign; a window that holds a negative value flags sum and avg, whose value
    is then the correctly rounded exact total: here every total is far below 2^53 in magnitude, so it equals the restatement's."""
    n = 600
    rng = np.random.default_rng(31)
    recs = make_recs(nf, addrs_v4(rng.integers(0, 12, n)))
    present = np.full(n, 7, dtype=np.uint8)
    parts = dict(additional=np.zeros(n, dtype=nf.ADDITIONAL), dns=np.zeros(n, dtype=nf.DNS), drops=np.zeros(n, dtype=nf.PKT_DROP))
    lat = rng.integers(-5 * 10**9, 5 * 10**9, n)
    lat[:6] = [-1, -999_999, -1_000_000, 0, 1_999_999, -2**63]                 # 0, 0, -1, 0, 1 ms; INT64_MIN ns
    parts["dns"]["latency"], parts["dns"]["id"] = lat.astype(np.int64).view(np.uint64), rng.integers(1, 65536, n)
    parts["drops"]["latest_drop_cause"], parts["drops"]["bytes"], parts["drops"]["packets"] = rng.integers(1, 80, n), rng.integers(0, 65536, n), rng.integers(0, 3, n)
    rtt = rng.integers(-2**40, 2**40, n)
    rtt[rtt == 0] = 1
    rtt[::50] = -2**63
    parts["additional"]["flow_rtt"] = rtt.astype(np.int64).view(np.uint64)
    keys = ("DnsLatencyMs", "PktDropBytes", "PktDropPackets", "TimeFlowRttNs")
    maps = content_maps(nf, recs, present, parts)
    assert all(all(k.encode() in m for k in keys) for m in maps) and min(m[b"DnsLatencyMs"] for m in maps) == -(2**63 // 10**6) and maps[2][b"DnsLatencyMs"] == -1
    exact_ops = ("min", "max", "count", "last", "diff")
    rules = [rule("%s %s" % (op, k), ["SrcAddr"], op, k, top=0 if j % 2 else 5, rev=bool(j % 3)) for j, k in enumerate(keys) for op in exact_ops[:4]]
    with Pair(nf, tab, rules, max_keys=16) as p:
        p.call(recs[:400], maps[:400], 1 * S, features=(present[:400], {k: v[:400] for k, v in parts.items()}))
        p.call(recs[400:], maps[400:], 2 * S, features=(present[400:], {k: v[400:] for k, v in parts.items()}))
    small = parts["additional"]["flow_rtt"].copy()
    small[::50] = np.int64(-7).view(np.uint64)                               # totals far below 2^53 in magnitude
    parts2 = dict(parts, additional=parts["additional"].copy())
    parts2["additional"]["flow_rtt"] = small
    rules = [rule("%s %s" % (op, k), ["SrcAddr"], op, k) for k in ("DnsLatencyMs", "TimeFlowRttNs") for op in ("sum", "avg", "diff", "last")] + \
            [rule("%s %s" % (op, k), ["SrcAddr"], op, k, top=4) for k in ("PktDropBytes", "PktDropPackets") for op in ("sum", "avg", "count")]
    lat2 = parts2["dns"]["latency"].copy()
    lat2[5] = np.int64(-3 * 10**6).view(np.uint64)
    parts2["dns"] = parts2["dns"].copy()
    parts2["dns"]["latency"] = lat2
    maps = content_maps(nf, recs, present, parts2)
    with Pair(nf, tab, rules, max_keys=16) as p:
        res, res_d = p.call(recs, maps, 1 * S, features=(present, parts2), flags_zero=False)
        for r, ru in enumerate(rules):
            signed_total = ru["operationType"] in ("sum", "avg") and ru["operationKey"] in ("DnsLatencyMs", "TimeFlowRttNs")
            for got in (res[r], res_d[r]):
                if signed_total:                                             # every key saw a negative value among its fifty flows
                    assert (got["flags"] == nf._lib.TB_INEXACT).all(), ru["name"]
                else:
                    assert not got["flags"].any(), ru["name"]
        # presence: a dns part without an id, a drops part without a cause
        parts2["dns"]["id"][3], parts2["drops"]["latest_drop_cause"][4] = 0, 0
        rc, _, _, missing = tab.timebased_extract(p.tbs[0], recs, 2 * S, None, None, (present, parts2), 64)
        assert (rc, missing) == (nf.EDEFER, 2)


def test_more_slices_than_the_cap(nf, tab):
    """NFAGG_TB_MAX_SLICES calls with flows inside one window: the next one is NFAGG_ERANGE and changes nothing; a call whose now
    puts enough of them outside the window is served, because the slices its own trim will drop do not count."""
    L = nf._lib
    rules = [rule("last", ["SrcAddr"], "last", interval=10 * S)]          # `last` merges no slice: the thousand calls stay quick
    recs = make_recs(nf, addrs_v4([1]), nbytes=3)
    with tab.timebased_rules(specs_of(nf, rules), None, None, 8) as tb:
        for k in range(L.TB_MAX_SLICES):
            rc, res, _, _ = tab.timebased_extract(tb, recs, k, None, None, None, 8)
            assert rc == nf.OK
        assert float(res[0]["value"][0]) == 3.0 and tb.stats().slices[0] == L.TB_MAX_SLICES
        with pytest.raises(nf.NfaggError) as e:
            tab.timebased_extract(tb, recs, L.TB_MAX_SLICES, None, None, None, 8)
        assert e.value.code == L.ERANGE and "live slices" in str(e.value)
        st = tb.stats()
        assert (st.slices[0], st.last_now_ns, st.keys[0]) == (L.TB_MAX_SLICES, L.TB_MAX_SLICES - 1, 1)
        rc, res, _, _ = tab.timebased_extract(tb, recs[:0], L.TB_MAX_SLICES, None, None, None, 8)       # without flows a call is always served
        assert rc == nf.OK and float(res[0]["value"][0]) == 3.0 and tb.stats().slices[0] == L.TB_MAX_SLICES
        now = 10 * S + 500                                                   # the slices stamped 0 .. 499 fall out of the window
        rc, res, _, _ = tab.timebased_extract(tb, recs, now, None, None, None, 8)
        assert rc == nf.OK and float(res[0]["value"][0]) == 3.0 and tb.stats().slices[0] == L.TB_MAX_SLICES - 500 + 1


# ---- 7. the deferral
def test_deferral_changes_nothing(nf, tab):
    n = 4097
    rng = np.random.default_rng(8)
    rules = [rule(op, ["SrcAddr"], op, top=0 if k % 2 else 20) for k, op in enumerate(OPS)] + [rule("pk", ["DstAddr"], "sum", "Packets")]
    first = make_recs(nf, addrs_v4(rng.integers(0, 300, 500)), nbytes=rng.integers(1, 10**6, 500))
    recs = make_recs(nf, addrs_v4(rng.integers(200, 900, n)), nbytes=rng.integers(1, 10**6, n))
    recs["metrics"]["bytes"][1234] = 0                                      # one zero-byte flow: it has Packets, so one table would take it
    with Pair(nf, tab, rules, max_keys=1024) as p:
        p.call(first, plain_maps(nf, first), 10 * S)
        before = [(tb.stats().keys[0], tb.stats().keys[1], tb.stats().slices[0], tb.stats().last_now_ns) for tb in p.tbs]
        rc, res, counts, missing = tab.timebased_extract(p.tbs[0], recs, 20 * S, None, None, None, 4096)
        rc_d, _, counts_d, missing_d = device_extract(nf, tab, p.tbs[1], recs, 20 * S, None, None, None, [4096] * len(rules))
        assert (rc, missing, counts) == (rc_d, missing_d, counts_d) == (nf.EDEFER, 1, [0] * len(rules)) and all(len(r) == 0 for r in res)
        assert [(tb.stats().keys[0], tb.stats().keys[1], tb.stats().slices[0], tb.stats().last_now_ns) for tb in p.tbs] == before
        # the caller drops the flow and repeats, at an EARLIER stamp than the refused call's: the clock did not move either. The
        # restatement never saw the refused call.
        keep = np.arange(n) != 1234
        p.call(recs[keep], plain_maps(nf, recs[keep]), 15 * S)


# ---- 8. overflow
@pytest.mark.parametrize("entry", ["host", "device"])
def test_key_overflow(nf, tab, entry):
    import torch
    rules = [rule("sum", ["SrcAddr"], "sum")]
    if entry == "host":
        extract = lambda tb, recs, now, cap: tab.timebased_extract(tb, recs, now, None, None, None, cap)  # noqa: E731
        results = lambda tb, cap: tab.timebased_results(tb, cap)  # noqa: E731
    else:
        extract = lambda tb, recs, now, cap: device_extract(nf, tab, tb, recs, now, None, None, None, [cap])  # noqa: E731
        results = lambda tb, cap: tab.timebased_results_device(tb, [cap], [torch.zeros(cap * 16, dtype=torch.uint8, device="cuda").data_ptr()])  # noqa: E731
    with tab.timebased_rules(specs_of(nf, rules), None, None, 64) as tb:
        ok = make_recs(nf, addrs_v4(np.arange(64)))
        rc, res, counts, _ = extract(tb, ok, 1 * S, 64)
        assert rc == nf.OK and counts == [64]
        over = make_recs(nf, addrs_v4(np.arange(65)))                       # max_keys + 1 keys
        rc, res, counts, _ = extract(tb, over, 2 * S, 128)
        assert rc == nf.TRUNCATED and counts == [0] and tb.stats().failed == 1
        for call in (lambda: extract(tb, ok, 3 * S, 64), lambda: results(tb, 64), lambda: extract(tb, ok[:0], 3 * S, 64)):
            with pytest.raises(nf.NfaggError) as e:
                call()
            assert e.value.code == nf._lib.EINVAL and "nfagg_timebased_reset" in str(e.value)
        tb.reset()
        st = tb.stats()
        assert (st.failed, st.has_clock, st.keys[0], st.slices[0]) == (0, 0, 0, 0)
        rc, res, counts, _ = extract(tb, ok, 0, 64)                         # the clock starts again too
        assert rc == nf.OK and counts == [64] and sorted(res[0]["value"].tolist()) == [1.0] * 64
    with tab.timebased_rules(specs_of(nf, rules), None, None, 64) as tb:      # far more keys than slots: the walk ends early
        rc, _, counts, _ = tab.timebased_extract(tb, make_recs(nf, addrs_v4(np.arange(20_000))), 1 * S, None, None, None, 64)
        assert rc == nf.TRUNCATED and tb.stats().failed == 1


# ---- 9. a results buffer that is too small
def test_small_results_buffer(nf, tab):
    rules = [rule("all", ["SrcAddr"], "sum"), rule("top", ["SrcAddr"], "sum", top=10), rule("count", ["DstAddr"], "count")]
    rng = np.random.default_rng(12)
    with Pair(nf, tab, rules, max_keys=256) as p:
        first = make_recs(nf, addrs_v4(rng.integers(0, 100, 300)), addrs_v4(rng.integers(0, 7, 300)), nbytes=rng.integers(1, 1000, 300))
        p.call(first, plain_maps(nf, first), 1 * S)
        recs = make_recs(nf, addrs_v4(rng.integers(50, 200, 300)), addrs_v4(rng.integers(0, 7, 300)), nbytes=rng.integers(1, 1000, 300))
        p.ref.extract(plain_maps(nf, recs), 2 * S)
        n_keys, n_dst = len(p.ref.filters[0]["results"]), len(p.ref.filters[2]["results"])
        caps = [n_keys - 1, 10, n_dst]
        rc, res, counts, _ = tab.timebased_extract(p.tbs[0], recs, 2 * S, None, None, None, caps)
        rc_d, res_d, counts_d, _ = device_extract(nf, tab, p.tbs[1], recs, 2 * S, None, None, None, caps)       # its canaries: nothing written
        assert rc == rc_d == nf.TRUNCATED and counts == counts_d == [n_keys, 10, n_dst] and all(len(r) == 0 for r in res + res_d)
        assert p.tbs[0].stats().failed == 0 and p.tbs[0].stats().slices[0] == 2 and p.tbs[0].stats().last_now_ns == 2 * S      # the state HAS advanced
        rc, res, counts = tab.timebased_results(p.tbs[0], [n_keys, 10, n_dst])
        assert rc == nf.OK and counts == [n_keys, 10, n_dst]
        import torch
        d_outs = [torch.zeros(c * 16, dtype=torch.uint8, device="cuda") for c in (n_keys, 10, n_dst)]
        rc_d, counts_d = tab.timebased_results_device(p.tbs[1], [n_keys, 10, n_dst], [o.data_ptr() for o in d_outs])
        torch.cuda.synchronize()
        assert rc_d == nf.OK and counts_d == counts
        for r in range(3):
            check_rule(nf, p.tbs[0], r, rules, res[r], p.ref)
            check_rule(nf, p.tbs[1], r, rules, d_outs[r].cpu().numpy().view(nf.TB_RESULT), p.ref)
        later = make_recs(nf, addrs_v4([1]))
        p.call(later, plain_maps(nf, later), 3 * S)                         # and the next call goes on from there


def test_call_checks(nf, tab):
    rules = [rule("sum", ["SrcAddr"], "sum"), rule("ns", ["SrcK8S_Namespace"], "sum"), rule("dir", ["FlowDirection"], "sum")]
    recs = make_recs(nf, addrs_v4([1, 2]))
    with tab.k8s_table([("10.0.0.1", dict(namespace="a", name="x", kind="Pod"))]) as k8s, tab.timebased_rules(specs_of(nf, rules), k8s, None, 8) as tb:
        rows = tab.k8s_resolve(k8s, recs)
        net_rows = np.zeros(2, dtype=nf.NET_ROW)
        with pytest.raises(nf.NfaggError) as e:
            tab.timebased_results(tb, 8)
        assert e.value.code == nf._lib.ESTATE
        for kr, nr, needle in ((None, net_rows, "needs the flows' k8s rows"), (rows, None, "needs the flows' net rows")):
            with pytest.raises(nf.NfaggError) as e:
                tab.timebased_extract(tb, recs, 5, kr, nr, None, 8)
            assert e.value.code == nf._lib.EINVAL and needle in str(e.value)
        assert tab.timebased_extract(tb, recs, 5, rows, net_rows, None, 8)[0] == nf.OK
        with pytest.raises(nf.NfaggError) as e:
            tab.timebased_extract(tb, recs, 4, rows, net_rows, None, 8)
        assert e.value.code == nf._lib.EINVAL and "below the previous call's" in str(e.value)
        with pytest.raises(nf.NfaggError) as e:
            tb.keys(0, [2])
        assert "not below the table's 2 keys" in str(e.value)
        assert tab.timebased_extract(tb, recs[:0], 5, None, None, None, 8)[0] == nf.OK          # n == 0 needs no rows


# ---- 10. the stage
def test_the_stage_end_to_end(nf, tab, world):
    recs, entries, maps = world
    cfg = dict(rules=[
        dict(name="top talkers", indexKeys=["SrcAddr"], operationType="sum", operationKey="Bytes", topK=10, timeInterval="30s"),
        dict(name="namespaces", indexKeys=["SrcK8S_Namespace", "DstK8S_Namespace"], operationType="sum", operationKey="Bytes", topK=10, timeInterval="1m"),
        dict(name="skipped", operationType="sum", operationKey="Bytes"),
        dict(name="quiet", indexKey="DstSubnetLabel", operationType="avg", operationKey="Packets", topK=2, reversed=True, timeInterval="10s"),
        dict(name="all", indexKeys=["Proto", "FlowDirection"], operationType="count", operationKey="Packets", timeInterval="10s"),
    ])
    ref = T.Timebased([dict(r, timeInterval=nf.conntrack.parse_duration(r.get("timeInterval") or 0)) for r in cfg["rules"]])
    with tab.k8s_table(entries, LAYER) as k8s, NC.net_table(nf, ALL, tab) as net, nf.ExtractTimebased(tab, cfg, k8s, net, max_keys=512, agent_ip=REPORTER) as stage:
        assert [it["name"] for it, _ in stage.skipped] == ["skipped"]
        for k, (now, lo, hi) in enumerate(((100 * S, 0, 120), (105 * S, 100, 300), (111 * S, 0, 0), (140 * S, 290, 300), (171 * S, 0, 0))):
            got = stage.extract(recs[lo:hi], now)
            want = ref.extract(maps[lo:hi], now)
            at = 0
            for r, f in enumerate(ref.filters):
                mine, theirs = got[at:at + len(ref.per_rule[r])], ref.per_rule[r]
                at += len(theirs)
                opkey = f["rule"]["operationKey"]
                assert len(mine) == len(theirs) and all(set(m) == set(t) and all(isinstance(v, (str, float)) for v in m.values()) for m, t in zip(mine, theirs))
                key_of = lambda m: ",".join(m[c] for c in f["rule"]["indexKeys"])  # noqa: E731
                if f["rule"].get("topK"):
                    assert all(T.same_bits(m[opkey], t[opkey]) for m, t in zip(mine, theirs)), (k, r)
                    assert len({key_of(m) for m in mine}) == len(mine) and all(T.same_bits(m[opkey], f["results"][key_of(m)]) for m in mine)
                else:
                    assert {key_of(m): m[opkey] for m in mine} == {key_of(t): t[opkey] for t in theirs}
                assert all((m["name"], m["index_key"], m["operation"]) == (t["name"], t["index_key"], t["operation"]) for m, t in zip(mine, theirs))
            assert at == len(got) == len(want) and not any(stage.inexact)
        none = recs[np.isin(recs["metrics"]["eth_protocol"], (0x0800, 0x86DD))][:5].copy()
        none["metrics"]["bytes"] = 0
        with pytest.raises(nf.MissingOperationKey) as e:
            stage.extract(none, 172 * S)
        assert e.value.count == 5
    with nf.ExtractTimebased(tab, dict(rules=cfg["rules"][:1]), max_keys=4) as small:
        with pytest.raises(nf.TimebasedOverflow):
            small.extract(recs, 1)
        small.reset()
        assert len(small.extract(recs[:1], 1)) <= 1
    for bad, needle in ((dict(indexKeys=["SrcMac"], operationType="sum", operationKey="Bytes"), "'SrcMac' is not served"),
                        (dict(indexKeys=["SrcAddr"], operationType="sum", operationKey="DnsId"), "operation key 'DnsId'"),
                        (dict(indexKeys=["SrcK8S_Name"], operationType="sum", operationKey="Bytes"), "needs the Kubernetes table")):
        with pytest.raises(ValueError) as e:
            nf.ExtractTimebased(tab, [bad])
        assert needle in str(e.value)
