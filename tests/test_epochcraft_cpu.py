"""CPU only. tests/epochcraft.py itself: every call that tests/test_crafted_epochs_gpu.py feeds the kernels is what its plan says —
the preconditions of the GPU tests as checked facts:

  the planned cuts are epoch_cuts(prev_links(...)) (tests/test_epoch_boundaries.py), as many as the oracle's evictions on full;
  the numpy model of the epochs-found-first path (tests/test_epoch_segments.py, 1024 lanes as the kernel has) gives the oracle's
  middle evictions from them;
  the designed segments count the asked number of sorted positions under the model's sort keys, on the intended side of
  kSegShort and kSegHuge; collider pairs share their hash bits; the record that was designed to decide a field does."""
import numpy as np
import pytest

import epochcraft as ec
import keycraft as kc
import test_epoch_segments as ts
from test_epoch_boundaries import epoch_cuts, prev_links

CONSTS = ec.constants()
NAMES = list(ec.cases(CONSTS))
_FACTS = {}


def facts(O, name):
    """Everything the checks below look at, computed once per call: the oracle's evictions, the model's sort keys, links, cuts
    and middle evictions."""
    if name in _FACTS:
        return _FACTS[name]
    call = ec.get(O, name)
    recs, M = call.recs, call.max_entries
    want = O.run_accounter(call.everything(), M)
    kid = ts.key_ids(call.everything())
    n_live = 0 if call.live_recs is None else len(call.live_recs)
    live_ids = np.unique(kid[:n_live])
    kid = kid[n_live:]
    ks = ts.sort_keys(O, recs, 0xFFFFFFFFFFFFFFFF)
    prev, over = ts.links(ks, kid, CONSTS["kLinkSearch"])
    assert not over, "the link search's bound: the call would be declined"
    rule_live = (np.isin(kid, live_ids), len(live_ids)) if n_live else None
    rule_cuts = epoch_cuts(prev_links(kid), M, rule_live)
    walk_prev = prev.copy()
    if n_live:
        walk_prev[(prev == -1) & np.isin(kid, live_ids)] = -2         # k_par_live
    cuts, tail_flows = ts.cut_walk(walk_prev, M, len(live_ids), 65535, CONSTS["kCutBlock"], CONSTS["kCutPer"])
    middle = []
    if len(cuts) >= 2:
        pos = ts.ranks(walk_prev, cuts, M)
        out, _ = ts.fold_segments(O, recs, ks, kid, pos, cuts, M)
        ev = out.reshape(-1).view(O.FLOW_RECORD).reshape(len(cuts) - 1, M)
        middle = [ts.sort_records(e) for e in ev]
    _FACTS[name] = dict(call=call, want=want, ks=ks, prev=walk_prev, rule_cuts=rule_cuts, cuts=cuts, tail_flows=tail_flows, middle=middle,
                        live0=len(live_ids))
    return _FACTS[name]


def test_the_constants_are_the_sources():
    c = CONSTS
    assert (c["S"], c["H"], c["C"]) == (16, 4096, 2048) and (c["row"], c["wave"], c["block"]) == (256, 1024, 16384)
    assert (c["chain_block"], c["chain_window"]) == (256, 16384) and c["kLinkSearch"] == 4096


@pytest.mark.parametrize("name", NAMES)
def test_planned_cuts_are_the_rules_and_the_oracles(O, name):
    f = facts(O, name)
    call = f["call"]
    assert call.live0 == f["live0"]
    assert f["rule_cuts"] == call.cuts, "the prefix-count rule cuts elsewhere"
    assert f["cuts"] == call.cuts, "the model of the cut walk cuts elsewhere"
    want = f["want"]
    assert [r for r, _ in want] == ["full"] * len(call.cuts) + ["closing"]
    assert all(len(ev) == call.max_entries for _, ev in want[:-1]) and f["tail_flows"] == len(want[-1][1])
    assert CONSTS["par_min"] <= len(call.recs) <= 70_000 + 152
    # prev == -1 is not all the walk sees: a third of the heads after the first epoch are flows the call has seen before
    if name.startswith(("cuts_", "live_")) and len(call.cuts) >= 2:
        a, b = call.cuts[0], call.cuts[-1]
        starts = np.asarray(call.cuts)[np.searchsorted(call.cuts, np.arange(a, b), side="right") - 1]
        head = f["prev"][a:b] < starts
        seen_before = head & (f["prev"][a:b] != -1)
        print("%s: %d heads in the middle epochs, %d with a previous occurrence in the call" % (name, head.sum(), seen_before.sum()))
        assert 3 * seen_before.sum() >= head.sum()


@pytest.mark.parametrize("name", NAMES)
def test_the_model_folds_the_middle_epochs_to_the_oracles(O, name):
    f = facts(O, name)
    assert len(f["middle"]) == max(0, len(f["call"].cuts) - 1)
    for t, g in enumerate(f["middle"]):
        assert f["want"][t + 1][0] == "full"
        assert g.tobytes() == ts.sort_records(f["want"][t + 1][1]).tobytes(), "middle epoch %d" % t


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith(("seg_", "field_"))])
def test_designed_segments_have_the_asked_positions(O, name):
    f = facts(O, name)
    call = f["call"]
    S, H = CONSTS["S"], CONSTS["H"]
    seen = set()
    for seg in call.info["segments"]:
        assert call.cuts[seg["epoch"] - 1] == seg["lo"] and call.cuts[seg["epoch"]] == seg["hi"]
        in_epoch = call.flow[seg["lo"]:seg["hi"]]
        assert (in_epoch == seg["hot"]).sum() == seg["L"] and (call.flow == seg["hot"]).sum() == seg["L"]
        assert len(np.unique(in_epoch)) == call.max_entries
        head = seg["lo"] + int(np.nonzero(in_epoch == seg["hot"])[0][0])
        positions = ec.segment_positions(f["ks"], head, seg["hi"])
        if seg["c"]:
            assert (in_epoch == seg["col"]).sum() == seg["c"]
            chead = seg["lo"] + int(np.nonzero(in_epoch == seg["col"])[0][0])
            assert chead > head                                        # the hot flow's head is the run's first position
            w = kc.as_words(call.keys[[seg["hot"], seg["col"]]])
            hh = kc.key_hash(w)
            assert hh[0] == hh[1] and (w[0] != w[1]).any()             # one 64-bit hash (so: one set of 40 hash bits), two keys
            cpos = ec.segment_positions(f["ks"], chead, seg["hi"])
            hot_after = int((in_epoch[chead - seg["lo"]:] == seg["hot"]).sum())
            assert cpos == seg["c"] + hot_after
            seg["col_class"] = ec.seg_class(cpos, CONSTS)
        assert positions == seg["L"] + seg["c"], (seg, positions)
        seg["class"] = ec.seg_class(positions, CONSTS)
        seen.add((seg["class"], ec.seg_class(seg["L"], CONSTS)))
        print("%s epoch %d: L %d c %d -> %d positions, %s%s" % (name, seg["epoch"], seg["L"], seg["c"], positions, seg["class"],
                                                                  (", collider " + seg["col_class"]) if seg["c"] else ""))
    by = {(s["L"], s["c"]): s for s in call.info["segments"]}
    if name == "seg_lengths":
        cls = {s["L"]: s["class"] for s in call.info["segments"]}
        assert [cls[x] for x in (S - 1, S, S + 1, H, H + 1)] == ["short", "short", "long", "long", "huge"]
        assert cls[1] == cls[2] == "short" and cls[2 * H + 1] == "huge"
    if name == "seg_positions":
        # by positions on the far side of the threshold, by records on the near side — and the collider the longer one
        assert {("long", "short"), ("huge", "long")} <= seen
        assert by[(5, 2 * S)]["col_class"] == "long" and by[(S + 4, H - 10)]["col_class"] == "huge"
    if name == "seg_inside":
        got = {(s["class"], s["col_class"]) for s in call.info["segments"]}
        assert {("long", "long"), ("huge", "huge"), ("long", "short")} <= got
    if name == "seg_sketch":
        assert {s["class"] for s in call.info["segments"]} == {"short", "long", "huge"}
    if name.startswith("field_"):
        want_class = {"field_short": "short", "field_long": "long"}.get(name, "huge")
        assert {s["class"] for s in call.info["segments"]} == {want_class}


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("field_")])
def test_the_designed_record_decides_the_field(O, name):
    f = facts(O, name)
    call = f["call"]
    kinds = set()
    for seg in call.info["segments"]:
        r = call.recs[seg["idx"]]
        by_rule = ec.rule_fold(r)
        ev = f["want"][seg["epoch"]][1]
        raw = np.ascontiguousarray(ev).view(np.uint8).reshape(len(ev), 144)
        hit = np.nonzero((raw[:, :39] == call.keys[seg["hot"], :39]).all(axis=1))[0]
        assert len(hit) == 1
        got = ec.fields_of(ev[hit[0]])
        assert got == by_rule, (seg["kind"], seg["nz"])                # the rules restated here are the oracle's
        for field, v in seg["expect"].items():
            assert got[field] == v, (seg["kind"], seg["nz"], field)
        if seg["kind"] == "nz":
            others = np.delete(np.arange(len(r)), seg["nz"])
            for field in ec.ORDER_FIELDS:
                assert not np.asarray(r["metrics"][field][others]).any()
            assert all(got[field] for field in ec.ORDER_FIELDS)
            if len(seg["nz"]) == 2:                                    # "the last" is not "the largest", "the first" not "the smallest"
                a, b = (ec.fields_of(r[k]) for k in seg["nz"])
                assert a["dscp"] > b["dscp"] and a["eth_protocol"] > b["eth_protocol"] and a["sampling"] > b["sampling"]
                assert a["src_mac"] < b["src_mac"] and a["dst_mac"] < b["dst_mac"]
                assert a["end"] > b["end"] and (a["end"] & 0xFFFFFFFF) < (b["end"] & 0xFFFFFFFF) and a["start"] > b["start"]
        if seg["kind"] == "head_zero":
            assert not any(ec.fields_of(r[0])[field] not in (0, bytes(6)) for field in ec.ORDER_FIELDS)
        kinds.add((seg["kind"], len(seg["nz"])))
    assert {("nz", 1), ("nz", 2), ("start_only", 1), ("end_high", 2), ("head_zero", 0)} <= kinds or name.startswith("field_huge")


def test_every_field_variant_reaches_the_huge_fold(O):
    kinds, ks = set(), set()
    for name in [n for n in NAMES if n.startswith("field_huge")]:
        for seg in ec.get(O, name).info["segments"]:
            kinds.add((seg["kind"], len(seg["nz"])))
            if seg["kind"] == "nz" and len(seg["nz"]) == 1:
                ks.add(seg["nz"][0])
    H, C = CONSTS["H"], CONSTS["C"]
    assert {("nz", 1), ("nz", 2), ("start_only", 1), ("end_high", 2), ("head_zero", 0)} <= kinds
    assert ks == {0, 1, 63, 64, 65, 255, 256, C - 1, C, H - 1, H, H + C + 299}      # both sides of every chunk's edge, the last record


def test_cut_positions_cover_the_walks_geometry(O):
    G, R, W, B = (CONSTS[k] for k in ("group", "row", "wave", "block"))
    per_m = {}
    for name in [n for n in NAMES if n.startswith("cuts_m")]:
        call = ec.get(O, name)
        per_m.setdefault(call.max_entries, set()).update(call.cuts)
    assert sorted(per_m) == [1, 2, 5, ec.BIG_M]
    for M, cuts in per_m.items():
        assert {R - 1, R, R + 1, W - 1, W, W + 1, B - 1, B, B + 1, 4 * B - 1, 4 * B} <= cuts, M
        assert {c % G for c in cuts} == set(range(G))
    q = [c for c in per_m[1] if c // G == 40000 // G]
    assert len(q) == G                                                # four consecutive cuts inside one group of four
    s = ec.get(O, "cuts_straddle").cuts
    assert any(a // G == B // G - 1 and b // G == B // G for a, b in zip(s, s[1:]))      # a block's last group to the next block's first
    call = ec.get(O, "cuts_quiet_blocks")
    a, b = call.cuts[3:5]
    prev = facts(O, "cuts_quiet_blocks")["prev"]
    new = np.nonzero(prev[a:b] < a)[0] + a
    assert len(new) == call.max_entries and new.max() < B and b >= 3 * B and a % G      # blocks 1 and 2 hold no new flow of the epoch
    assert ec.get(O, "cuts_last_record").cuts[-1] == len(ec.get(O, "cuts_last_record").recs) - 1
    assert [len(ec.get(O, n).recs) for n in ("cuts_exact_block", "cuts_block_plus_1", "cuts_four_blocks")] == [B, B + 1, 4 * B]
    t = ec.get(O, "cuts_truncated")
    assert t.deliver[0] // t.max_entries == 2 and len(t.recs) - t.cuts[-1] >= CONSTS["par_min"]      # every resumed call stays above the entry bar


def test_live_families(O):
    full = ec.get(O, "live_full_new")
    assert full.live0 == full.max_entries and full.cuts[0] == 0 and full.flow[0] >= full.live0
    j = ec.get(O, "live_full_after_7")
    assert j.live0 == j.max_entries and j.cuts[0] == 7 and (j.flow[:7] < j.live0).all() and j.flow[7] >= j.live0
    part = ec.get(O, "live_part")
    first, later = part.flow[:part.cuts[0]], part.flow[part.cuts[0]:]
    assert 0 < part.live0 < part.max_entries and (first < part.live0).any() and (later < part.live0).any()
    for name, per_side in (("live_one_home", ec.ONE_HOME_K // 2), ("live_edges", 4), ("live_same64", 1)):
        call = ec.get(O, name)
        sp = call.info["special"]
        live, new = [x for x in sp if x < call.live0], [x for x in sp if x >= call.live0]
        assert len(live) == len(new) == per_side
        # the special flows that are not live appear first in the account call's FIRST epoch (that is where k_par_live decides)
        firsts = {int(x): int(np.nonzero(call.flow == x)[0][0]) for x in new}
        assert max(firsts.values()) < call.cuts[0]
        hl, hn = kc.key_hash(kc.as_words(call.keys[live])), kc.key_hash(kc.as_words(call.keys[new]))
        if name == "live_one_home":
            assert len(set(hl.tolist()) | set(hn.tolist())) == ec.ONE_HOME_K
            assert all(int(x) & ec.ONE_HOME_LOW == ec.ONE_HOME_LOW for x in np.concatenate([hl, hn]))
        else:
            assert sorted(hl.tolist()) == sorted(hn.tolist())
        if name == "live_edges":
            assert sorted(int(x) for x in hl) == sorted(ec.EDGE_HASHES)


# ---------------------------------------------------------------- are the families sharp? The kernels' arithmetic, restated, with ONE thing wrong
# Nothing below runs a kernel. cut_block's counting (nfagg_epoch_par.hip) is restated at the level where its edges are — groups of
# four records per lane, the group that holds an epoch's start — and SegAcc's tagged words as they are; then one comparison or
# constant is changed in the RESTATEMENT and the calls of the GPU file must tell: a family that a wrong variant passes is not sharp.
NEVER = 0x7fffffff


def walk_by_groups(prev, max_entries, live0, wrong=None, expect=None):
    """k_par_cuts / cut_block: blocks of kCutBlock * kCutPer records; of the resident block the records of every group of four
    that is not WHOLLY before the epoch's start s are compared (first epoch: prev == -1, later: prev < s); the lane that holds s
    overwrites its records before s with "never new" when the cut is made. wrong = "keep_dead": no overwrite; "round_up": the
    number of dead groups rounded up, (s - row_base + 3) >> 2. expect: the walk stops at its first cut that is not expect's (a wrong
    walk may cut at nearly every record)."""
    span, G = CONSTS["block"], CONSTS["group"]
    n = len(prev)
    s, before, first = 0, 0, True
    budget = 0 if live0 >= max_entries else max_entries - live0
    cuts = []
    for b in range((n + span - 1) // span):
        idx = np.arange(b * span, (b + 1) * span)
        cur = np.full(span, NEVER, dtype=np.int64)
        cur[:min(n, (b + 1) * span) - b * span] = prev[b * span:(b + 1) * span]
        while True:
            dead_groups = (s + G - 1) // G if wrong == "round_up" else s // G
            counted = ((idx // G) >= dead_groups) & ((cur == -1) if first else (cur < s))
            total = int(counted.sum())
            if before + total <= budget:
                before += total
                break
            f = int(idx[np.nonzero(counted)[0][budget - before]])
            cuts.append(f)
            if expect is not None and cuts != expect[:len(cuts)]:
                return cuts
            s, before, first, budget = f, 0, False, max_entries
            if wrong != "keep_dead":
                cur[(idx // G == f // G) & (idx < f)] = NEVER
    return cuts


def test_the_restated_walk_is_the_plans_and_wrong_walks_are_not(O):
    caught = {"keep_dead": [], "round_up": []}
    names = [n for n in NAMES if n.startswith(("cuts_", "live_"))]
    for name in names:
        f = facts(O, name)
        call = f["call"]
        assert walk_by_groups(f["prev"], call.max_entries, f["live0"], None, call.cuts) == call.cuts, name
        for wrong in caught:
            if walk_by_groups(f["prev"], call.max_entries, f["live0"], wrong, call.cuts) != call.cuts:
                caught[wrong].append(name)
    for wrong, got in caught.items():
        print("%s: %d of %d calls cut elsewhere: %s" % (wrong, len(got), len(names), " ".join(got)))
    # Records before s in the group of four that holds s: kept alive they count again (prev < own index < s), with the dead groups
    # rounded up the epoch's own first record is lost — either way the NEXT cut moves, wherever a cut that is not the call's last
    # falls on a record index that is no multiple of four. Every such call must tell, and that is most of them.
    G = CONSTS["group"]
    must = [n for n in names if any(c % G for c in ec.get(O, n).cuts[:-1])]
    for wrong, got in caught.items():
        assert set(must) <= set(got), (wrong, sorted(set(must) - set(got)))
    assert {"cuts_m1_0", "cuts_m2_0", "cuts_m5_0", "cuts_m%d_0" % ec.BIG_M, "cuts_straddle", "cuts_quiet_blocks", "cuts_last_record", "cuts_exact_block",
            "cuts_block_plus_1", "cuts_four_blocks", "cuts_truncated", "live_full_after_7"} <= set(must)


def seg_acc(r, idx, wrong=None):
    """SegAcc (nfagg_epoch_par.hip) over the records r of one flow with call indices idx, combined in a scrambled order: tagged
    words (index + 1) << width | value, the largest wins; MACs by the smallest index. wrong = "dscp_largest": the tag without
    the index."""
    m = r["metrics"]
    order = np.random.default_rng(len(r)).permutation(len(r))
    end = start_inv = eth = dscp = samp = 0
    smac_at = dmac_at = 1 << 32
    smac = dmac = bytes(6)
    for j in order:
        i, s1 = int(idx[j]), int(idx[j]) + 1
        end = max(end, int(m["end"][j]))
        if int(m["start"][j]):
            start_inv = max(start_inv, ec.M64 ^ int(m["start"][j]))
        if int(m["eth_protocol"][j]):
            eth = max(eth, (s1 << 16) | int(m["eth_protocol"][j]))
        if int(m["dscp"][j]):
            dscp = max(dscp, ((0 if wrong == "dscp_largest" else s1) << 8) | int(m["dscp"][j]))
        if int(m["sampling"][j]):
            samp = max(samp, (s1 << 32) | int(m["sampling"][j]))
        if m["src_mac"][j].any() and i < smac_at:
            smac_at, smac = i, bytes(m["src_mac"][j])
        if m["dst_mac"][j].any() and i < dmac_at:
            dmac_at, dmac = i, bytes(m["dst_mac"][j])
    return {"start": (ec.M64 ^ start_inv) if start_inv else 0, "end": end, "eth_protocol": eth & 0xFFFF, "dscp": dscp & 0xFF,
            "sampling": samp & 0xFFFFFFFF, "src_mac": smac, "dst_mac": dmac}


@pytest.mark.parametrize("name", ["field_long", "field_huge_0", "field_huge_1", "field_huge_2"])
def test_the_order_free_partials_and_a_wrong_one(O, name):
    call = ec.get(O, name)
    told = []
    for seg in call.info["segments"]:
        r = call.recs[seg["idx"]]
        assert seg_acc(r, seg["idx"]) == ec.rule_fold(r), (seg["kind"], seg["nz"])
        wrong = seg_acc(r, seg["idx"], "dscp_largest")
        if any(wrong[f] != v for f, v in seg["expect"].items()):
            told.append((seg["kind"], tuple(seg["nz"])))
    print("%s: the largest DSCP instead of the last is told by %s" % (name, told))
    pairs = [(s["kind"], tuple(s["nz"])) for s in call.info["segments"] if s["kind"] == "nz" and len(s["nz"]) == 2]
    assert set(pairs) <= set(told) and (pairs or name == "field_huge_0")      # every two-record variant tells


def test_a_live_check_by_hash_alone_moves_the_cuts(O):
    """par_is_live compares the key behind a matching tag. Restated without that compare (a first occurrence counts as live when
    its HASH is a live flow's), the calls with one hash live and new cut elsewhere."""
    moved = []
    for name in [n for n in NAMES if n.startswith("live_")]:
        f = facts(O, name)
        call = f["call"]
        live_h = set(kc.key_hash(kc.as_words(call.keys[:call.live0])).tolist())
        h = kc.key_hash(kc.as_words(call.keys[call.flow]))
        prev = f["prev"].copy()
        prev[(prev == -1) & np.isin(h, list(live_h))] = -2
        if walk_by_groups(prev, call.max_entries, f["live0"], None, call.cuts) != call.cuts:
            moved.append(name)
    print("live by hash alone: cuts move in", moved)
    assert {"live_edges", "live_same64"} <= set(moved)
