"""tests/partcraft.py on the CPU: the families have the sizes they name, the oracle's per-CPU folds (orc_rollup) and its map merge
equal a restatement of the six Accumulate* and of buildBaseFromAdditional in plain Python integers — written from
pkg/model/flow_content.go:63-198 and pkg/tracer/tracer.go:1057-1146, not from the oracle's C — on every script, the embedded ones
included, and the families have TEETH: each single-rule mutant of the restatement is told from the truth by the family built for
its rule."""
import numpy as np
import pytest

import partcraft as pc

M16, M64 = 0xFFFF, (1 << 64) - 1
SIZES = {"additional": 6174, "dns": 6174, "drops": 4368, "quic": 1884, "xlat": 16275, "netev": 6174, "ring": 2000}
MUTANTS = {"additional": ["ret compared unsigned", "rtt compared signed"], "dns": ["latency compared signed", "errno kept when the other is zero"],
           "drops": ["drops wrapping"], "xlat": ["xlat replaced when one address is non-zero", "the near-miss taken for zero"],
           "netev": ["netev duplicates appended"], "ring": ["netev duplicates appended"]}


# ---------------------------------------------------------------- the restatement (dicts of Python integers and lists)
def signed64(v):
    return v - (1 << 64) if v >> 63 else v


def add_uint16(a, b):
    s = (a + b) & M16
    return M16 if s < a else s


def build_base(b, o):
    """buildBaseFromAdditional (flow_content.go:63-74)."""
    if b["start"] == 0 or (b["start"] > o["start"] and o["start"] != 0):
        b["start"] = o["start"]
    if b["end"] == 0 or b["end"] < o["end"]:
        b["end"] = o["end"]
    if b["eth_protocol"] == 0:
        b["eth_protocol"] = o["eth_protocol"]


def all_zero_ip(a, mutant):
    """AllZeroIP (record.go:233-238): net.IP.Equal takes the IPv4-mapped form of 0.0.0.0 for IPv4zero."""
    if mutant == "the near-miss taken for zero" and not any(a[:10]) and a[11] == 0xff and not any(a[12:]):
        return True
    return not any(a) or (not any(a[:10]) and a[10] == 0xff and a[11] == 0xff and not any(a[12:]))


def acc_dns(p, o, mutant, trace):
    p["flags"] |= o["flags"]
    if o["id"] != 0:
        p["id"] = o["id"]
    if p["err_no"] != o["err_no"] and not (mutant == "errno kept when the other is zero" and o["err_no"] == 0):
        p["err_no"] = o["err_no"]
    less = signed64(p["latency"]) < signed64(o["latency"]) if mutant == "latency compared signed" else p["latency"] < o["latency"]
    if less:
        p["latency"] = o["latency"]


def acc_drops(p, o, mutant, trace):
    if mutant == "drops wrapping":
        p["bytes"], p["packets"] = (p["bytes"] + o["bytes"]) & M16, (p["packets"] + o["packets"]) & M16
    else:
        p["bytes"], p["packets"] = add_uint16(p["bytes"], o["bytes"]), add_uint16(p["packets"], o["packets"])
    p["latest_flags"] |= o["latest_flags"]
    if o["latest_drop_cause"] != 0:
        p["latest_drop_cause"] = o["latest_drop_cause"]
    if o["latest_state"] != 0:
        p["latest_state"] = o["latest_state"]


def acc_netev(p, o, mutant, trace):
    for i, md in enumerate(o["network_events"]):
        exists = md in p["network_events"] and mutant != "netev duplicates appended"
        if o["packets"][i] != 0 and exists and not any(md) and trace is not None:
            trace["zero_taken_for_present"] += 1
        if o["packets"][i] != 0 and not exists:
            at = p["network_events_idx"]
            if trace is not None:
                old = p["network_events"][at]
                trace["reappeared"] += md in trace.setdefault("gone", [])
                if any(old) or p["packets"][at] or p["bytes"][at]:
                    trace["gone"].append(old)
                    trace["reused"] += 1
                    trace["saturated_in_reused"] += (p["bytes"][at] + o["bytes"][i] > M16) or (p["packets"][at] + o["packets"][i] > M16)
                trace["wrapped"] += at == 3
            p["bytes"][at] = add_uint16(p["bytes"][at], o["bytes"][i])
            p["packets"][at] = add_uint16(p["packets"][at], o["packets"][i])
            p["network_events"][at] = list(md)
            p["network_events_idx"] = (at + 1) % 4


def acc_xlat(p, o, mutant, trace):
    zs, zd = all_zero_ip(o["saddr"], mutant), all_zero_ip(o["daddr"], mutant)
    if (not zs or not zd) if mutant == "xlat replaced when one address is non-zero" else (not zs and not zd):
        p.clear()
        p.update(o)


def acc_additional(p, o, mutant, trace):
    less = signed64(p["flow_rtt"]) < signed64(o["flow_rtt"]) if mutant == "rtt compared signed" else p["flow_rtt"] < o["flow_rtt"]
    if less:
        p["flow_rtt"] = o["flow_rtt"]
    key = (lambda v: v & 0xFFFFFFFF) if mutant == "ret compared unsigned" else (lambda v: v)
    if key(p["ipsec_ret"]) < key(o["ipsec_ret"]):
        p["ipsec_encrypted"], p["ipsec_ret"] = o["ipsec_encrypted"], o["ipsec_ret"]
    if p["ipsec_ret"] == o["ipsec_ret"]:
        if o["ipsec_encrypted"]:
            p["ipsec_encrypted"] = o["ipsec_encrypted"]


def acc_quic(p, o, mutant, trace):
    for f in ("version", "seen_long_hdr", "seen_short_hdr"):
        if p[f] < o[f]:
            p[f] = o[f]


ACC = {"dns": acc_dns, "drops": acc_drops, "network_events": acc_netev, "xlat": acc_xlat, "additional": acc_additional, "quic": acc_quic}


def accumulate(kind, base, part, o, mutant=None, trace=None):
    """p.Accumulate<Kind>(other): the base first, then the stored partial — the first CPU's is stored whole. Returns the partial."""
    build_base(base, o)
    if part is None:
        return {k: ([list(x) for x in v] if isinstance(v, list) and v and isinstance(v[0], list) else list(v) if isinstance(v, list) else v) for k, v in o.items()}
    ACC[kind](part, o, mutant, trace)
    return part


def rows(a):
    """A structured array as one dict of Python values per element."""
    names = a.dtype.names
    plain = lambda v: v.tolist() if isinstance(v, np.ndarray) else v          # noqa: E731 (sub-array fields come back as arrays)
    return [{k: plain(v) for k, v in zip(names, r)} for r in np.asarray(a).reshape(-1).tolist()]


def fold_call(call, mutant=None, trace=None):
    """orc_rollup's job from the Go text: per flow the CPUs in ascending order. Returns [(base dict, part dict)]."""
    parts, out = rows(call.parts), []
    for f, base in enumerate(rows(call.base)):
        part = None
        t = None if trace is None else dict.fromkeys(("zero_taken_for_present", "reappeared", "reused", "saturated_in_reused", "wrapped"), 0)
        for o in parts[f * call.n_cpu:(f + 1) * call.n_cpu]:
            part = accumulate(call.kind, base, part, o, mutant, t)
        if trace is not None:
            for k in trace:
                trace[k] += t[k] > 0
        out.append((base, part))
    return out


def as_arrays(call, folded):
    def tup(d):
        return tuple(tuple(map(tuple, v)) if isinstance(v, list) and v and isinstance(v[0], list) else tuple(v) if isinstance(v, list) else v for v in d.values())
    return (np.array([tup(b) for b, _ in folded], dtype=call.base.dtype), np.array([tup(p) for _, p in folded], dtype=call.parts.dtype))


# ---------------------------------------------------------------- the builder
@pytest.mark.parametrize("name", pc.FAMILIES)
def test_families_have_the_sizes_the_issue_names(name):
    fam = pc.family(name)
    assert fam.n_scripts == SIZES[name] == len(np.unique(fam.keys, axis=0))
    if name == "ring":
        assert [c.n_cpu for c in fam.calls] == [8]
        idx = fam.calls[0].parts["network_events_idx"]
        assert idx.min() == 0 and idx.max() == 3
        return
    n = pc.N_SYMBOLS[name]
    assert [c.n_cpu for c in fam.calls] == [1, 2, 3, 5, 6, 7, 8, 9] and [len(c.script) for c in fam.calls] == [n, n * n] + [n ** 3] * 6
    assert len(set(fam.seqs)) == fam.n_scripts and {len(s) for s in fam.seqs} == {1, 2, 3}
    for c in fam.calls[3:]:                                              # embedded: CPUs (0, k, n_cpu - 1), everything else zero
        raw = c.parts.view(np.uint8).reshape(len(c.script), c.n_cpu, -1)
        used = np.zeros((len(c.script), c.n_cpu), dtype=bool)
        used[np.arange(len(c.at))[:, None], c.at] = True
        assert not raw[~used].any() and (c.at[:, 0] == 0).all() and (c.at[:, 2] == c.n_cpu - 1).all()
        assert np.array_equal(c.at[:, 1], 1 + c.script % (c.n_cpu - 2)) and set(c.at[:, 1].tolist()) == set(range(1, c.n_cpu - 1))
        assert c.parts[np.arange(len(c.at))[:, None], c.at].tobytes() == fam.calls[2].parts.tobytes()
    three = fam.calls[2]
    assert {(int(s), int(e)) for s, e in zip(three.parts["start"].reshape(-1), three.parts["end"].reshape(-1))} == {(a, b) for a in pc.TIMES for b in pc.TIMES}
    assert set(three.base["start"].tolist()) == set(pc.TIMES) and (three.parts["eth_protocol"] == 0).any() and (three.parts["eth_protocol"] != 0).any()


def test_symbols_by_their_fields():
    """What the issue's table lists, read back from the partials of the length-1 scripts (symbol k = script k)."""
    one = lambda name: pc.family(name).calls[0].parts[:, 0]                  # noqa: E731
    a = one("additional")
    assert sorted(set(zip(a["ipsec_ret"].tolist(), a["ipsec_encrypted"].tolist(), a["flow_rtt"].tolist()))) == sorted(
        (r, e, t) for r in (-(1 << 31), 0, (1 << 31) - 1) for e in (0, 1) for t in (0, 5, 1 << 63))
    d = one("dns")
    assert sorted(set(zip(d["id"].tolist(), d["err_no"].tolist(), d["latency"].tolist()))) == sorted(
        (i, e, t) for i in (0, 7, 0xFFFF) for e in (0, 5) for t in (0, 9, 1 << 63))
    assert (d["flags"] == 1).all() and (d["name"] == 0x61).all()
    two = pc.family("dns").calls[1].parts
    assert (two["flags"][:, 1] == 2).all() and (two["name"][:, 1] == 0x62).all() and set(two["id"][:, 1].tolist()) == {0, 8, 0xFFFE}
    r = one("drops")
    assert set(zip(r["bytes"].tolist(), r["packets"].tolist())) == {(0, 0xFFFF), (1, 0x8000), (0x8000, 1), (0xFFFF, 0)}
    assert set(zip((r["latest_drop_cause"] != 0).tolist(), (r["latest_state"] != 0).tolist())) == {(False, False), (True, False), (False, True), (True, True)}
    q = one("quic")
    assert sorted(set(zip(q["version"].tolist(), q["seen_long_hdr"].tolist(), q["seen_short_hdr"].tolist()))) == sorted(
        (v, s, 255 if s == 0 else 0 if s == 255 else 1) for v in (0, 1, 1 << 31, (1 << 32) - 1) for s in (0, 1, 255))
    x = one("xlat")
    assert len({(bytes(s), bytes(t)) for s, t in zip(x["saddr"], x["daddr"])}) == 25
    assert bytes(pc.FORMS[3]) == bytes(10) + b"\x00\xff" + bytes(4) and bytes(pc.FORMS[4]) == bytes.fromhex("20010db8000000000000000000000001")
    e = one("netev")
    slot = np.where(np.arange(18) < 9, 0, 3)
    assert sorted(set(zip(slot.tolist(), [bytes(m) for m in e["network_events"][np.arange(18), slot]], e["packets"][np.arange(18), slot].tolist()))) == sorted(
        (s, bytes(m), p) for s in (0, 3) for m in pc.MD for p in (0, 1, 0xFFFF))
    assert np.array_equal(pc.family("netev").calls[2].parts["network_events_idx"][:, 0], pc.family("netev").calls[2].script % 4)


# ---------------------------------------------------------------- the oracle equals the restatement
@pytest.mark.parametrize("name", pc.FAMILIES)
def test_oracle_rollup_equals_the_python_restatement(O, name):
    fam = pc.family(name)
    for call in fam.calls:
        want_base, want_part = as_arrays(call, fold_call(call))
        got_base, got_part = O.rollup(call.kind, call.parts, call.n_cpu, call.base)
        for what, g, w in (("base", got_base, want_base), ("folded", got_part, want_part)):
            bad = np.nonzero((g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)).any(axis=1))[0]
            assert len(bad) == 0, "%s, n_cpu %d, %s: %d flows differ, first %s" % (name, call.n_cpu, what, len(bad), fam.describe(int(call.script[bad[0]])))


def python_walk(w, order=pc.WALK):
    """LookupAndDeleteMap's join (tracer.go:1022-1146) on a Walk: {key bytes: (base dict, {kind: part dict})}."""
    flows = {}
    for i, v in zip(w.main_ids, rows(w.main_vals)):
        flows[i.tobytes()] = (v, {})
    zero = rows(np.zeros(1, dtype=w.main_vals.dtype))[0]
    for kind in order:
        ids, vals = w.feats[kind]
        for i, per_cpu in zip(ids, vals):
            base, parts = flows.setdefault(i.tobytes(), (dict(zero), {}))
            for o in rows(per_cpu):
                parts[kind] = accumulate(kind, base, parts.get(kind), o)
    return flows


@pytest.mark.parametrize("n_cpu", [1, 2])
def test_oracle_map_merge_walks_the_maps_in_the_tracers_order(O, n_cpu):
    w = pc.walk(n_cpu)
    ids, contents = O.map_merge(w.main_ids, w.main_vals, w.feats, n_cpu)
    truth, enum_order = python_walk(w), python_walk(w, pc.ENUM)
    assert len(ids) == w.n_flows == len(truth)
    told = 0
    for i, c in zip(ids, contents):
        base, parts = truth[i.tobytes()]
        s = int(np.nonzero((w.keys[:, :39] == np.frombuffer(i.tobytes(), dtype=np.uint8)[:39]).all(axis=1))[0][0])
        assert rows(c["base"])[0] == base, s
        first = w.first_map(s)
        assert base["eth_protocol"] == (0x1000 + pc.ENUM.index(first) if first else 0)
        for kind, has, field in (("dns", "has_dns", "dns"), ("drops", "has_drops", "drops"), ("network_events", "has_netev", "netev"),
                                 ("xlat", "has_xlat", "xlat"), ("additional", "has_additional", "additional"), ("quic", "has_quic", "quic")):
            assert bool(c[has]) == (kind in parts), (s, kind)
            if kind in parts:
                assert rows(c[field])[0] == parts[kind], (s, kind)
        told += enum_order[i.tobytes()][0] != base
    print("\nwalk, n_cpu %d: walk in enum order told apart by %d of %d flows" % (n_cpu, told, len(ids)))
    assert told > 0


# ---------------------------------------------------------------- the families have teeth
@pytest.mark.parametrize("name", list(MUTANTS))
def test_every_mutant_is_told_apart_by_its_family(name):
    fam = pc.family(name)
    print()
    for mutant in MUTANTS[name]:
        differ = []
        for call in fam.calls[:3]:
            differ += [int(call.script[f]) for f, (a, b) in enumerate(zip(fold_call(call, mutant), fold_call(call))) if a != b]
        print("%-10s %-44s told apart by %5d of %5d scripts%s" % (name, mutant, len(differ), fam.n_scripts, ", first " + fam.describe(differ[0]) if differ else ""))
        assert differ, "%s: no script of %s tells it from the truth" % (mutant, name)


def test_ring_reaches_what_it_was_built_for():
    trace = dict.fromkeys(("zero_taken_for_present", "reappeared", "reused", "saturated_in_reused", "wrapped"), 0)
    fold_call(pc.family("ring").calls[0], trace=trace)
    print("\nring, scripts that reach each case:", trace)
    assert trace["wrapped"] > 100                  # the index wraps past 3
    assert trace["reappeared"] > 20                # an overwritten metadata value reappears and is appended again
    assert trace["zero_taken_for_present"] > 20    # all-zero metadata with packets meets an empty slot and is taken for present
    assert trace["saturated_in_reused"] > 20       # a saturating add lands in a reused slot
