"""transform filter on the GPU (nfagg_filter_apply, nfagg_gather; csrc/nfagg_filter.h, nfagg_filter.hip) through the C ABI, host
and device entry points: keep, rule, kept_idx and out_records exactly against the per-flow restatement of
tests/flp_filter_ref.py over the enriched maps of the other restatements; the filter, the gather and the direct-FLP JSON
encoder composed against the restatement's lines of the kept maps. Records, parts, namer table and informer answers are those
of the transform network tests."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_filter_ref as FR  # noqa: E402
import flp_json_content_ref as RC  # noqa: E402
import flp_json_k8s_ref as K  # noqa: E402
import flp_json_net_ref as R  # noqa: E402
import flp_json_tls_ref as RT  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_flp_json_k8s_gpu as KG  # noqa: E402
import test_flp_json_net_cpu as NC  # noqa: E402
import test_flp_json_net_gpu as NG  # noqa: E402
import test_flp_json_tls_gpu as TG  # noqa: E402
import test_netev_gpu as E  # noqa: E402
from flp_json_ref import marshal_sorted, record_to_map  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, NOW, MONO, RECEIVED = G.NAMES, G.NOW, G.MONO, G.RECEIVED
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 66_563]          # 66 563: more than 64 scan blocks and a ragged tail
RULES = dict(direction=True, labels=NG.CATEGORIES, flags=False)      # Flags stays a number
RULES_NAMES = dict(RULES, flags=True)                                # Flags is a []string
N_FULL = 331


def keep(q, sampling=0):
    return dict(type="keep_entry_query", keepEntryQuery=q, keepEntrySampling=sampling)


def rm(t, key, **v):
    return dict(type=t, removeEntry=dict(input=key, **v))


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


class World:
    """One batch with everything around it: records of every shape with their parts, both tables, the resolved rows, and the
    enriched maps of the restatements, computed once."""

    def __init__(self, nf, O, tab, rules):
        recs, present, parts, _ = TG.policy_inputs(nf, O, N_FULL, 71, 1)
        recs = recs.copy()
        m = recs["metrics"]
        m["ssl_version"], m["tls_cipher_suite"], m["tls_key_share"] = 0, 0, 0
        m["bytes"][3], m["bytes"][4], m["bytes"][5] = 2**63, 2**63 - 1, 2**64 - 1          # negative as int, the largest int, -1
        samp = [0, 1, 65537, 65538, 2, 0xFFFFFFFF, 4294967295 // 65535, 4294967295 // 65535 + 1]
        m["sampling"] = np.array([samp[i % len(samp)] for i in range(N_FULL)], dtype=np.uint32)
        self.recs, self.present, self.parts, self.rules = recs, present, parts, rules
        self.entries = KG.entries_for(recs)
        self.k8s = tab.k8s_table(self.entries, KG.LAYER)
        self.net = NC.net_table(nf, rules, tab)
        self.k8s_rows = tab.k8s_resolve(self.k8s, recs)
        self.net_rows = tab.net_resolve(self.net, recs, self.k8s, self.k8s_rows, NG.REPORTER)
        self.tls_ref = RT.table_of(nf.GO_TLS_NAMES)
        cats = R.parse_subnets(rules["labels"])
        table, memo = K.table_of(self.entries), {}
        raw = recs.view(np.uint8).reshape(-1, 144)
        self.maps = []
        for i in range(N_FULL):
            rec = raw[i].tobytes()
            mp = RT.add_tls(record_to_map(rec, NOW, MONO, G.rows(NAMES), NG.REPORTER, RECEIVED, b"unknown", memo), rec, self.tls_ref)
            RC.add_content(mp, RC.flow_parts(present, parts, i))
            self.maps.append(R.apply_rules(mp, table, KG.LAYER, rules, cats))

    def compile(self, nf, cfg):
        return nf.TransformFilter(cfg, k8s_entries=self.entries, labels=self.net.labels, layer=True, net_flags=self.net.flags)

    def close(self):
        self.net.close()
        self.k8s.close()


@pytest.fixture(scope="module")
def world(nf, O, tab):
    w = World(nf, O, tab, RULES)
    yield w
    w.close()


@pytest.fixture(scope="module")
def world_names(nf, O, tab):
    w = World(nf, O, tab, RULES_NAMES)
    yield w
    w.close()


def want_records(recs, idx, kept_maps, keep):
    """The kept records, sampling rewritten from the kept maps except where the flow is deferred."""
    out = recs[idx].copy()
    for j, (i, mp) in enumerate(zip(idx, kept_maps)):
        if keep[i] == 1:
            out["metrics"]["sampling"][j] = mp.get(b"Sampling", 0)
    return out


def device_apply(nf, tab, flt, recs, k8s_rows=None, net_rows=None, features=None, seed=0, first=0, cap=None):
    """nfagg_filter_apply_device into buffers with canaries behind them."""
    import torch
    n = len(recs)
    cap = n if cap is None else cap
    d_recs = E.dev(recs) if n else None
    d_k = E.dev(k8s_rows) if k8s_rows is not None and n else None
    d_n = E.dev(net_rows) if net_rows is not None and n else None
    d_feat = None
    if features is not None and n:
        d_p = E.dev(features[0])
        d_parts = {k: E.dev(v) for k, v in features[1].items()}
        d_feat = (d_p.data_ptr(), {k: v.data_ptr() for k, v in d_parts.items()})
    d_keep = torch.full((n + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    d_rule = torch.full((n + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    d_idx = torch.full((cap + 16,), -1, dtype=torch.int32, device="cuda")
    d_out = torch.full(((cap + 1) * 144,), 0xAB, dtype=torch.uint8, device="cuda")
    ptr = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
    rc, n_kept, n_def = tab.filter_apply_device(flt, ptr(d_recs), n, ptr(d_k), ptr(d_n), d_feat, NOW, MONO, seed, first, d_keep.data_ptr(), d_rule.data_ptr(),
                                                d_idx.data_ptr(), d_out.data_ptr(), cap)
    torch.cuda.synchronize()
    keep_, rule, idx, out = d_keep.cpu().numpy(), d_rule.cpu().numpy(), d_idx.cpu().numpy().view(np.uint32), d_out.cpu().numpy()
    assert (keep_[n:] == 0xAB).all() and (rule[n:] == 0xAB).all()
    wrote = n_kept if rc == nf.OK else 0
    assert (idx[wrote:] == 0xFFFFFFFF).all() and (out[wrote * 144:] == 0xAB).all()       # nothing behind the kept, nothing at all when truncated
    return rc, keep_[:n], rule[:n], idx[:wrote], out[:wrote * 144].view(nf.FLOW_RECORD), n_kept, n_def


def check_against(nf, tab, w, cfg, maps=None, recs=None, seed=0, first=0, device=True, rows=True, features=True):
    """Compile, apply through the host entry point (and the device one), compare with the restatement. Returns the host result."""
    maps = w.maps if maps is None else maps
    recs = w.recs if recs is None else recs
    keep_, rule, idx, kept = FR.run(cfg, maps, nf.parse_query, seed, first)
    kw = dict(k8s_rows=w.k8s_rows if rows else None, net_rows=w.net_rows if rows else None, features=(w.present, w.parts) if features else None)
    with tab.filter(w.compile(nf, cfg), w.k8s, w.net) as flt:
        got = tab.filter_apply(flt, recs, now_unix_ns=NOW, mono_now_ns=MONO, seed=seed, first_index=first, **kw)
        dev = device_apply(nf, tab, flt, recs, seed=seed, first=first, **kw) if device else None
    want_out = want_records(recs, idx, kept, keep_)
    for g in (got, dev) if dev is not None else (got,):
        assert g[0] == nf.OK and g[5] == len(idx) and g[6] == keep_.count(2)
        assert g[1].tolist() == keep_ and g[2].tolist() == rule and g[3].tolist() == idx
        assert g[4].tobytes() == want_out.tobytes()
    return got, keep_


# ---- sizes and keep patterns: the scan and the compaction
def pattern(name, n):
    i = np.arange(n)
    return {"all": i >= 0, "none": i < 0, "alternating": i % 2 == 0, "lane": i % 64 == 37, "block": i % 1024 == 1000, "first": i == 0, "last": i == n - 1}[name]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_keep_patterns(nf, O, tab, n):
    base = G.stream(nf, O, n, seed=n + 3).copy()
    cfg = dict(rules=[keep("Bytes = 7")])
    with tab.filter(nf.TransformFilter(cfg)) as flt:
        for name in ("all", "none", "alternating", "lane", "block", "first", "last"):
            recs = base.copy()
            sel = pattern(name, n)
            recs["metrics"]["bytes"] = np.where(sel, 7, np.where(recs["metrics"]["bytes"] == 7, 8, recs["metrics"]["bytes"]))
            keep_, rule, idx, _ = FR.run(cfg, FR.light_maps(recs), nf.parse_query)
            assert idx == np.flatnonzero(sel).tolist()                          # the restatement and the pattern agree
            got = tab.filter_apply(flt, recs)
            assert got[0] == nf.OK and got[1].tolist() == keep_ and got[2].tolist() == rule and got[3].tolist() == idx and got[5:] == (len(idx), 0)
            assert got[4].tobytes() == recs[idx].tobytes()
            if name in ("alternating", "lane", "last"):
                dev = device_apply(nf, tab, flt, recs)
                assert dev[0] == nf.OK and all(np.array_equal(a, b) for a, b in zip(got[1:4], dev[1:4])) and got[4].tobytes() == dev[4].tobytes()
                assert dev[5:] == got[5:]
            if name == "alternating" and len(idx) > 1:                          # NFAGG_TRUNCATED with the exact count, nothing written
                for fn in (lambda cap: tab.filter_apply(flt, recs, cap=cap), lambda cap: device_apply(nf, tab, flt, recs, cap=cap)):
                    short = fn(len(idx) - 1)
                    assert short[0] == nf.TRUNCATED and short[5] == len(idx) and len(short[3]) == 0 and short[1].tolist() == keep_
                    exact = fn(len(idx))
                    assert exact[0] == nf.OK and exact[3].tolist() == idx


def test_a_spec_with_no_steps_keeps_everything(nf, O, tab):
    recs = G.stream(nf, O, 200, seed=9)
    with tab.filter(nf.TransformFilter(dict(rules=[]))) as flt:
        got = tab.filter_apply(flt, recs)
        assert got[0] == nf.OK and got[1].tolist() == [1] * 200 and got[2].tolist() == [FR.NO_RULE] * 200 and got[3].tolist() == list(range(200))
        assert got[4].tobytes() == recs.tobytes()
        none = tab.filter_apply(flt, recs, out_records=False, cap=0)             # neither kept_idx nor out_records asked for: the count alone
        assert none[0] == nf.OK and none[5] == 200 and none[1].tolist() == [1] * 200


# ---- every field, present and absent shapes
NUM_KEYS = ["Etype", "Bytes", "Packets", "Sampling", "Proto", "Dscp", "SrcPort", "DstPort", "IcmpType", "IcmpCode", "Flags", "TimeFlowStartMs",
            "TimeFlowEndMs", "FlowDirection", "TimeFlowRttNs", "DnsLatencyMs", "DnsId", "DnsFlags", "DnsErrno", "PktDropBytes", "PktDropPackets",
            "PktDropLatestFlags", "IPSecRetCode"]


@pytest.mark.parametrize("key", NUM_KEYS)
def test_every_num_field(nf, tab, world, key):
    vals = sorted({FR.convert_to_int(m[key.encode()])[0] for m in world.maps if key.encode() in m})
    have = sum(key.encode() in m for m in world.maps)
    assert 0 < have and (have < N_FULL or key in ("Etype", "TimeFlowStartMs", "TimeFlowEndMs")), "present and absent shapes"
    mid, lo, hi = (max(v, 0) for v in (vals[len(vals) // 2], vals[0], vals[-1]))         # the language has no negative literal
    for q in ("%s = %d" % (key, mid), "%s != %d" % (key, mid), "%s < %d" % (key, mid), "%s > %d" % (key, mid), "%s <= %d" % (key, lo), "%s >= %d" % (key, hi),
              "with(%s)" % key, "without(%s)" % key, '%s = "%d"' % (key, mid), '%s != "%d"' % (key, mid), "%s < 0 or %s >= 0" % (key, key)):
        got, want = check_against(nf, tab, world, dict(rules=[keep(q)]), device=q.startswith("with"))
        if q.startswith(("with(", key + " = %d" % mid)):
            assert 0 < sum(want) <= N_FULL


def test_bytes_at_two_to_the_63_is_negative(nf, tab, world):
    got, want = check_against(nf, tab, world, dict(rules=[keep("Bytes < 0")]))
    assert want[3] == 1 and want[4] == 0 and want[5] == 1 and sum(want) >= 2


def test_flags_under_decode_tcp_flags(nf, tab, world_names):
    for q, some in (("Flags > 0", False), ("Flags <= 0", False), ("Flags != 0", False), ('Flags = "SYN"', False), ("with(Flags)", True), ('Flags != "SYN"', True)):
        got, want = check_against(nf, tab, world_names, dict(rules=[keep(q)]))
        assert (sum(want) > 0) == some


def test_presence_only_fields_addresses_and_macs(nf, tab, world):
    ip = next(m for m in world.maps if b"SrcAddr" in m and b":" in m[b"SrcAddr"])
    v4 = next(m for m in world.maps if b"DstAddr" in m and b"." in m[b"DstAddr"])
    q = ('SrcAddr = "%s" or DstAddr = "%s" or SrcMac = "%s" or DstMac = "%s" and without(DstAddr) or SrcAddr = "::ffff:1.2.3.4"'
         % (ip[b"SrcAddr"].decode(), v4[b"DstAddr"].decode(), world.maps[7][b"SrcMac"].decode(), world.maps[8][b"DstMac"].decode()))
    got, want = check_against(nf, tab, world, dict(rules=[keep(q)]))
    assert sum(want) >= 2
    for q in ("with(SrcAddr)", "without(DstAddr)", "with(SrcMac) and without(Interfaces)", 'SrcAddr != "%s"' % ip[b"SrcAddr"].decode()):
        check_against(nf, tab, world, dict(rules=[keep(q)]), device=False)


# ---- table atoms
def test_table_atoms_and_not_of_no_row(nf, tab, world):
    qs = ['SrcK8S_Name =~ "^obj-1"', 'DstK8S_Namespace != "%s"' % KG.INFOS[0].get("namespace", ""), "without(SrcK8S_Name)", 'SrcK8S_Name !~ "obj"',
          "with(DstK8S_Zone) and without(SrcK8S_HostName)", 'SrcSubnetLabel = "low v4" or DstSubnetLabel =~ "high"', "without(SrcSubnetLabel)",
          'K8S_FlowLayer = "app"', 'K8S_FlowLayer != "infra"', 'DnsFlagsResponseCode = "NoError" or DnsFlagsResponseCode =~ "^N"', "without(DnsFlagsResponseCode)",
          'IPSecStatus = "error"', 'IPSecStatus != "success"', "with(IPSecStatus)", "SrcK8S_Name > 5", "FlowDirection = 1 or FlowDirection = 2"]
    some = 0
    for q in qs:
        got, want = check_against(nf, tab, world, dict(rules=[keep(q)]), device=q.startswith("without(SrcK8S"))
        some += 0 < sum(want) < N_FULL
    assert some >= 12                                                            # the streams reach both answers of nearly every query
    assert sum(1 for m in world.maps if b"SrcK8S_Name" not in m) > 10            # "no row" is there to be negated


# ---- programs
def test_stack_of_32_and_64_atoms(nf, tab, world):
    deep = "Bytes = 0" + "".join(" or (Packets = %d" % k for k in range(31)) + ")" * 31
    spec = world.compile(nf, dict(rules=[keep(deep)]))
    assert len(spec.atoms) == 32
    check_against(nf, tab, world, dict(rules=[keep(deep)]))
    ports = sorted({m[b"SrcPort"] for m in world.maps if b"SrcPort" in m})
    wide = " or ".join("(SrcPort = %d and Proto = %d)" % (ports[k % len(ports)], (6, 17, 132)[k % 3]) for k in range(61))
    spec = world.compile(nf, dict(rules=[keep(wide)]))
    assert len(spec.atoms) == 64
    got, want = check_against(nf, tab, world, dict(rules=[keep(wide)]))
    assert 0 < sum(want) < N_FULL


def test_two_keep_rules_the_first_samples_out(nf, tab, world):
    cfg = dict(samplingField="Sampling", rules=[keep("with(Proto)", 3), keep("Proto = 6 or Proto = 17", 0), keep("without(Proto)", 2)])
    got, want = check_against(nf, tab, world, cfg, seed=11, first=1 << 40)
    rules = got[2].tolist()
    assert {0, 1, 2, FR.NO_RULE} <= set(rules)
    # consecutive calls with a running first_index roll differently, the same call rolls the same
    again, _ = check_against(nf, tab, world, cfg, seed=11, first=1 << 40, device=False)
    other, _ = check_against(nf, tab, world, cfg, seed=11, first=(1 << 40) + N_FULL, device=False)
    assert again[1].tolist() == got[1].tolist() and other[1].tolist() != got[1].tolist()


def test_remove_after_keep_sees_the_stored_sampling(nf, tab, world):
    cfg = dict(samplingField="Sampling", rules=[rm("remove_entry_if_doesnt_exist", "Sampling"), keep("with(Etype)", 4), keep("Packets > 0"),
                                                dict(type="remove_entry_all_satisfied", removeEntryAllSatisfied=[rm("remove_entry_if_exists", "Flags"),
                                                                                                                 rm("remove_entry_if_not_equal", "SrcK8S_Type", value="Pod")]),
                                                rm("remove_entry_if_equal", "Proto", value=6), rm("remove_entry_if_not_equal", "IcmpType", value=8)])
    got, want = check_against(nf, tab, world, cfg, seed=3)
    assert 0 < sum(1 for k in want if k) < N_FULL
    no_store = dict(cfg, samplingField="")
    got2, want2 = check_against(nf, tab, world, no_store, seed=3)
    assert want2 != want                                                         # without the store the first remove rule sees the record's own Sampling


def test_two_sample_if_groups(nf, tab, world):
    cfg = dict(rules=[dict(type="conditional_sampling", conditionalSampling=[dict(value=3, rules=[rm("remove_entry_if_exists", "SrcPort")]),
                                                                              dict(value=0, rules=[rm("remove_entry_if_exists", "Proto")]),
                                                                              dict(value=2, rules=[])]),
                      dict(type="conditional_sampling", conditionalSampling=[dict(value=2, rules=[rm("remove_entry_if_exists", "Bytes"),
                                                                                                  rm("remove_entry_if_doesnt_exist", "DnsId")]),
                                                                              dict(value=5, rules=[rm("remove_entry_if_equal", "K8S_FlowLayer", value="infra")])])])
    got, want = check_against(nf, tab, world, cfg, seed=99, first=12345)
    assert 0 < sum(want) < N_FULL and set(got[2].tolist()) == {FR.NO_RULE}


# ---- Sampling: stored, at the edges of 32 bits
EDGE = [0, 1, 65537, 65538, 2, 0xFFFFFFFF, 4294967295 // 65535, 4294967295 // 65535 + 1]


def test_sampling_store_multiplies_what_is_there(nf, tab, world):
    """World's records carry Sampling 0, 1, 65537, 65538, 2, 2^32 - 1 and the two values around (2^32 - 1) / 65535. With value 3
    about a third is admitted; the stored value is max(Sampling, 1) * 3, deferred where that needs more than 32 bits."""
    cfg = dict(samplingField="Sampling", rules=[keep("with(Etype)", 3)])
    got, want = check_against(nf, tab, world, cfg, seed=21)
    assert {0, 1, 2} == set(want) and got[6] == want.count(2) > 0
    kept = got[3].tolist()
    for j, i in enumerate(kept):
        s = int(world.recs["metrics"]["sampling"][i])
        assert int(got[4]["metrics"]["sampling"][j]) == (max(s, 1) * 3 if max(s, 1) * 3 <= 0xFFFFFFFF else s)


@pytest.mark.parametrize("s", EDGE)
def test_sampling_at_the_edge_of_32_bits(nf, tab, s):
    """keepEntrySampling 65535 over Sampling 0 and 1 (both store 65535), 65537 (65537 x 65535 = 2^32 - 1, the largest product that
    fits: stored), 65538 (does not fit: deferred, the record keeps its sampling), 2^32 - 1, and the largest Sampling whose
    product fits beside its successor. The flow sits at an index the roll admits."""
    cfg = dict(samplingField="Sampling", rules=[keep("Bytes = 1", 65535)])
    first = next(i for i in range(1 << 22) if FR.roll(5, i, 0, 65535))
    one = np.zeros(1, dtype=nf.FLOW_RECORD)
    one["metrics"]["bytes"], one["metrics"]["sampling"], one["metrics"]["eth_protocol"] = 1, s, 0x0806
    k, r, out = FR.transform(cfg, FR.light_maps(one)[0], nf.parse_query, 5, first)
    fits = max(s, 1) * 65535 <= 0xFFFFFFFF
    assert (k, r) == (1 if fits else 2, 0) and fits == (s in (0, 1, 2, 65537, 4294967295 // 65535))
    with tab.filter(nf.TransformFilter(cfg)) as flt:
        g = tab.filter_apply(flt, one, seed=5, first_index=first)
        miss = tab.filter_apply(flt, one, seed=5, first_index=first + 1)
    assert g[1].tolist() == [k] and g[2].tolist() == [0] and g[5:] == (1, 0 if fits else 1)
    assert int(g[4]["metrics"]["sampling"][0]) == (max(s, 1) * 65535 if fits else s) == (out[b"Sampling"] if fits else s)
    assert miss[1].tolist() == [0] and miss[2].tolist() == [FR.NO_RULE] and miss[5:] == (0, 0)


# ---- composition: filter, gather, encode
def lines_of(maps):
    return b"".join(marshal_sorted(m) + b"\n" for m in maps)


def test_filter_gather_encode_gives_the_lines_of_the_kept_maps(nf, tab, world):
    cfg = dict(samplingField="Sampling", rules=[keep("Proto = 6 and (SrcPort < 40000 or DstPort < 40000)", 2), keep('with(SrcK8S_Name) or SrcSubnetLabel = "low v4"'),
                                                rm("remove_entry_if_equal", "K8S_FlowLayer", value="nothing")])
    keep_, rule, idx, kept = FR.run(cfg, world.maps, nf.parse_query, 8, 1000)
    assert 20 < len(idx) < N_FULL - 20 and 0 in rule and 1 in rule
    fits = [j for j, i in enumerate(idx) if keep_[i] == 1]                       # a deferred flow is the host's to format
    with tab.filter(world.compile(nf, cfg), world.k8s, world.net) as flt:
        got = tab.filter_apply(flt, world.recs, world.k8s_rows, world.net_rows, (world.present, world.parts), NOW, MONO, 8, 1000)
    assert got[3].tolist() == idx
    out = got[4]
    g_present = tab.gather(world.present, got[3])
    g_parts = {k: tab.gather(v, got[3]) for k, v in world.parts.items()}
    assert g_present.tolist() == world.present[idx].tolist() and all(g_parts[k].tobytes() == world.parts[k][idx].tobytes() for k in g_parts)
    assert tab.gather(world.k8s_rows, got[3]).tolist() == world.k8s_rows[idx].tolist() == tab.k8s_resolve(world.k8s, out).tolist()
    assert tab.gather(world.net_rows, got[3]).tobytes() == world.net_rows[idx].tobytes()
    with tab.tls_names() as tls:
        buf, off = tab.encode_flp_json_net(out, tls, world.k8s, world.net, NOW, MONO, G.table(nf, NAMES), NG.REPORTER, RECEIVED, present=g_present, parts=g_parts)
    got_lines = [bytes(buf[int(off[j]):int(off[j + 1])]) for j in range(len(idx))]
    want_lines = [marshal_sorted(m) + b"\n" for m in kept]
    assert len(fits) > 10 and [got_lines[j] for j in fits] == [want_lines[j] for j in fits]
    stored = [j for j in fits if rule[idx[j]] == 0]
    assert stored and all(b'"Sampling":%d,' % kept[j][b"Sampling"] in got_lines[j] and kept[j][b"Sampling"] % 2 == 0 for j in stored)


def test_keep_all_leaves_the_encoder_output_as_it_was(nf, tab, world):
    with tab.filter(world.compile(nf, dict(rules=[keep("with(Etype)")])), world.k8s, world.net) as flt, tab.tls_names() as tls:
        got = tab.filter_apply(flt, world.recs)
        args = (tls, world.k8s, world.net, NOW, MONO, G.table(nf, NAMES), NG.REPORTER, RECEIVED)
        kw = lambda idx: dict(present=tab.gather(world.present, idx), parts={k: tab.gather(v, idx) for k, v in world.parts.items()})  # noqa: E731
        plain = tab.encode_flp_json_net(world.recs, *args, present=world.present, parts=world.parts)
        filtered = tab.encode_flp_json_net(got[4], *args, **kw(got[3]))
    assert got[5] == N_FULL and got[4].tobytes() == world.recs.tobytes()
    assert bytes(plain[0]) == bytes(filtered[0]) == lines_of(world.maps) and plain[1].tolist() == filtered[1].tolist()


# ---- the gather
@pytest.mark.parametrize("n", SIZES)
def test_gather_every_element_size(nf, tab, n):
    import torch
    rng = np.random.default_rng(n)
    idx = np.sort(rng.choice(n, size=n // 2, replace=False)).astype(np.uint32) if n else np.zeros(0, dtype=np.uint32)
    if n > 2:
        idx[-1] = n - 1                                                          # the last element too
    for elem in (1, 2, 4, 8, 16, 24, 32, 40, 48, 56, 64):
        src = rng.integers(0, 256, (n, elem), dtype=np.uint8)
        got = tab.gather(src, idx)
        assert got.shape == (len(idx), elem) and got.tobytes() == src[idx].tobytes()
        if n:
            # the device entry point, on the allocator's alignment and, for the sizes that move in 8-byte units or could move in
            # 16-byte ones, with source and destination 8 bytes off it: a multiple of 16 then goes in 8-byte units
            for shift in ((0, 8) if elem % 8 == 0 else (0,)):
                d_src = torch.zeros(n * elem + 16, dtype=torch.uint8, device="cuda")
                d_src[shift:shift + n * elem] = torch.from_numpy(src.reshape(-1)).cuda()
                d_idx = E.dev(idx)
                d_dst = torch.full((shift + len(idx) * elem + 64,), 0xAB, dtype=torch.uint8, device="cuda")
                assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
                tab.gather_device(d_src.data_ptr() + shift, n, elem, d_idx.data_ptr() if len(idx) else 0, len(idx), (d_dst.data_ptr() + shift) if len(idx) else 0)
                torch.cuda.synchronize()
                out = d_dst.cpu().numpy()
                assert out[shift:shift + len(idx) * elem].tobytes() == src[idx].tobytes()
                assert (out[:shift] == 0xAB).all() and (out[shift + len(idx) * elem:] == 0xAB).all()
    typed = rng.integers(0, 2**63, n, dtype=np.uint64)                           # hash ids keep their dtype and shape
    assert tab.gather(typed, idx).tolist() == typed[idx].tolist()


def test_gather_refusals_and_indexes_beyond_the_source(nf, tab):
    src = np.arange(40, dtype=np.uint32)
    beyond = tab.gather(src, np.array([0, 39, 40, 2**32 - 1], dtype=np.uint32))
    assert beyond.tolist() == [0, 39, 0, 0]                                      # an index from n_src up yields a zeroed element
    for elem in (3, 12, 72, 0):
        with pytest.raises(nf.NfaggError) as e:
            tab._check(nf._lib.lib.nfagg_gather(tab._h, src.ctypes.data, 4, elem, src.ctypes.data, 2, src.ctypes.data))
        assert e.value.code == nf._lib.EINVAL and "not 1, 2, 4, 8 or a multiple of 8 up to 64" in str(e.value)


def test_apply_refusals(nf, tab, world):
    spec = world.compile(nf, dict(rules=[keep('SrcK8S_Name = "obj-1" and FlowDirection = 1 and TimeFlowStartMs > 0')]))
    with tab.filter(spec, world.k8s, world.net) as flt:
        with pytest.raises(nf.NfaggError) as e:
            tab.filter_apply(flt, world.recs, None, world.net_rows)
        assert e.value.code == nf._lib.EINVAL and "reads the flows' Kubernetes rows" in str(e.value)
        with pytest.raises(nf.NfaggError) as e:
            tab.filter_apply(flt, world.recs, world.k8s_rows, None)
        assert "reads the flows' net rows" in str(e.value)
    with nf.Filter(nf.TransformFilter(dict(rules=[keep("Proto = 6")]))) as host_only:
        with pytest.raises(nf.NfaggError) as e:
            tab.filter_apply(host_only, world.recs)
        assert "was not created for this handle" in str(e.value)


# ---- the exporters take the stage
def test_direct_flp_json_with_a_filter(nf, tab, world):
    cfg = dict(samplingField="Sampling", rules=[keep("Proto = 6 or Proto = 17", 2), keep("with(SrcK8S_Name)")])
    held_lines = []

    def fallback(rec, now, mono, sampling):
        held_lines.append((int(rec["metrics"]["sampling"]), sampling))
        return b"HOST %d\n" % sampling

    with tab.filter(world.compile(nf, cfg), world.k8s, world.net) as flt, tab.tls_names() as tls:
        out = io.BytesIO()
        stage = nf.StageFilter(flt, seed=4)
        exp = nf.DirectFLPJSON(tab, out, G.table(nf, NAMES), NG.REPORTER, time_received=lambda: RECEIVED, tls_names=tls, k8s=world.k8s, net=world.net,
                               filter=stage, fallback=fallback)
        maps = [{k: v for k, v in m.items() if not k.startswith((b"Dns", b"PktDrop", b"IPSec", b"TimeFlowRtt", b"Xlat", b"Quic", b"ZoneId"))} for m in world.maps]
        want = b""
        for call in range(2):                                                    # evicted records carry no parts; the second call rolls on
            keep_, rule, idx, kept = FR.run(cfg, maps, nf.parse_query, 4, call * N_FULL)
            assert exp.ExportEvicted(world.recs, NOW, MONO) == len(idx)
            want += b"".join(b"HOST %d\n" % m[b"Sampling"] if keep_[i] == 2 else marshal_sorted(m) + b"\n" for i, m in zip(idx, kept))
        assert out.getvalue() == want and held_lines and stage.first_index == 2 * N_FULL and exp.deferred == len(held_lines)
        assert all(stored == 2 * own > 0xFFFFFFFF for own, stored in held_lines)     # the record keeps its sampling, the line's value comes beside it
    with pytest.raises(ValueError):
        nf.DirectFLPJSON(tab, io.BytesIO(), filter=object())


def test_map_tracer_with_a_filter(nf, O, tab):
    from test_map_merge import make_maps
    n_cpu = 4
    main_ids, main_vals, feats = make_maps(O, seed=11, n_pop=400, n_main=300, n_feat=250, n_cpu=n_cpu)
    main_vals["eth_protocol"] = 0x86DD
    main_vals["sampling"] = 3
    decoder = lambda cookie: None if cookie[0] % 2 == 0 else b"event %d" % cookie[1]  # noqa: E731
    mrecs, present, parts, _ = tab.map_merge(main_ids, main_vals, feats, n_cpu)
    entries = KG.entries_for(mrecs)
    mt = nf.MapTracer(nf.GPUMapFetcher(tab, lambda: (main_ids, main_vals, feats, n_cpu)), 0, 0, sample_decoder=decoder, clock=lambda: NOW, mono_clock=lambda: MONO)
    cfg = dict(samplingField="Sampling", rules=[keep("with(DnsId) or PktDropPackets > 100", 2), rm("remove_entry_if_doesnt_exist", "Packets")])
    with tab.tls_names() as tls, tab.k8s_table(entries, KG.LAYER) as k8s, NC.net_table(nf, NG.ALL, tab) as net:
        spec = nf.TransformFilter(cfg, k8s_entries=entries, labels=net.labels, layer=True, net_flags=net.flags)
        with tab.filter(spec, k8s, net) as flt:
            kw = dict(tls_names=tls, k8s=k8s, net=net)
            plain = mt.evictFlowsJSON(G.table(nf, NAMES), NG.REPORTER, RECEIVED, **kw)
            buf, off, held = mt.evictFlowsJSON(G.table(nf, NAMES), NG.REPORTER, RECEIVED, filter=nf.StageFilter(flt, seed=77), **kw)
            # the kept flows, from the product's own keep bytes: the stage's verdicts are checked above, here its place in the tracer
            p_out, dparts, rows, netev = mt.resolveNetworkEvents(present, parts)
            k8s_rows = tab.k8s_resolve(k8s, mrecs)
            got = tab.filter_apply(flt, mrecs, k8s_rows, tab.net_resolve(net, mrecs, k8s, k8s_rows, NG.REPORTER), (p_out, dparts), NOW, MONO, 77, 0)
    idx = got[3].tolist()
    assert held == [] and 10 < len(idx) < len(mrecs) - 10 and len(off) == len(idx) + 1
    lines = lambda b, o: [bytes(b[int(o[j]):int(o[j + 1])]) for j in range(len(o) - 1)]  # noqa: E731
    all_lines, kept_lines = lines(*plain), lines(buf, off)
    assert kept_lines == [all_lines[i].replace(b'"Sampling":3,', b'"Sampling":6,') for i in idx] and all(b'"Sampling":6,' in x for x in kept_lines)
