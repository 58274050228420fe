"""The six per-CPU part folds (pkg/model/flow_content.go:63-198; csrc/nfagg_rollup.hip k_rollup, and k_merge_fold through
fold_partials) on SCRIPTED partials. The other rollup tests draw random bytes at n_cpu 1, 8 and 80 — the four-way unrolled loop
then sees the tail lengths 0 and 3 only, ties and saturation edges happen by chance, and nothing pins the signed compare of
ipsec_encrypted_ret or the order in which the map merge walks the feature maps. tests/partcraft.py enumerates the orders of values
that matter; here every family goes through nfagg_rollup_* (one call per n_cpu: 1, 2, 3, and 5..9 with the partials embedded in
zero slices) at flow counts on both sides of a 256-lane workgroup, through nfagg_map_merge with every other flow in the main map,
and two of them through nfagg_map_merge_device — bit for bit against the oracle, which tests/test_partcraft_cpu.py holds against a
restatement of the Go text in Python integers on exactly these partials. A failure names the family, the script and the leg."""
import numpy as np
import pytest

import partcraft as pc
from test_map_merge import _assert_matches_oracle, _key40, _product_maps

pytestmark = pytest.mark.gpu

CUTS = (1, 255, 256, 257, None)             # flows per call: one, and both sides of a workgroup of 256 lanes; None: all
SIZES = {"records": 144, "present": 1, "additional": 32, "dns": 64, "drops": 32, "network_events": 72, "xlat": 56, "quic": 24}


def rows_differ(g, w):
    return np.nonzero((g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)).any(axis=1))[0]


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=16) as t:
        yield t


@pytest.mark.parametrize("name", pc.FAMILIES)
def test_rollup(nf, O, tab, name):
    """tab.rollup: one call per n_cpu and flow count. The oracle folds the whole call once; a cut call must give its prefix."""
    fam = pc.family(name)
    for call in fam.calls:
        want_base, want_part = O.rollup(call.kind, call.parts, call.n_cpu, call.base)
        for cut in CUTS:
            n = len(call.script) if cut is None else cut
            if n > len(call.script):
                continue
            got_base, got_part = tab.rollup(call.kind, call.parts[:n].view(np.uint8).reshape(-1).view(nf.ROLLUP_KINDS[call.kind]), call.n_cpu,
                                            call.base[:n].view(nf.FLOW_METRICS))
            for what, g, w in (("base metrics", got_base, want_base[:n]), ("folded partials", got_part, want_part[:n])):
                bad = rows_differ(g, w)
                assert len(bad) == 0, "%s, rollup, n_cpu %d, %d flows, %s: %d flows differ, first %s" % (
                    name, call.n_cpu, n, what, len(bad), fam.describe(int(call.script[bad[0]])))


def first_appearance(mi, feats):
    """The ids in the order the merge delivers them: main map rows first, then the ids new to each map in walk order."""
    seen, order = set(), []
    for ids in [mi] + [feats[k][0] for k in pc.WALK if k in feats]:
        for k in _key40(ids):
            if k.tobytes() not in seen:
                seen.add(k.tobytes())
                order.append(k.tobytes())
    return b"".join(order)


def check_merge(nf, O, got, mi, mv, feats, n_cpu, what):
    try:
        _assert_matches_oracle(nf, O, got, mi, mv, feats, n_cpu)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None
    assert got[0]["id"].tobytes() == first_appearance(mi, feats), what


@pytest.mark.parametrize("name", pc.FAMILIES)
def test_map_merge(nf, O, tab, name):
    """tab.map_merge: every script's partials in the family's feature map, a main-map row for the even scripts only — the odd
    ones start from zero base metrics (tracer.go:1138-1141)."""
    fam = pc.family(name)
    for call in fam.calls:
        mi, mv, feats = pc.merge_maps(fam, call)
        got = tab.map_merge(*_product_maps(nf, mi, mv, feats), call.n_cpu)
        assert got[3] == 0 and len(got[0]) == len(call.script)
        check_merge(nf, O, got, mi, mv, feats, call.n_cpu, "%s, map merge, n_cpu %d" % (name, call.n_cpu))


@pytest.mark.parametrize("n_cpu", [1, 2])
def test_map_merge_walks_the_maps_in_the_tracers_order(nf, O, tab, n_cpu):
    """Every subset of the six feature maps, with and without a main-map row: the merged eth_protocol is the FIRST map's of the
    walk dns, drops, network events, xlat, additional, quic (tracer.go:1057-1110) — not of NFAGG_ROLLUP_* order."""
    w = pc.walk(n_cpu)
    got = tab.map_merge(*_product_maps(nf, w.main_ids, w.main_vals, w.feats), n_cpu)
    assert len(got[0]) == w.n_flows
    check_merge(nf, O, got, w.main_ids, w.main_vals, w.feats, n_cpu, "walk, n_cpu %d" % n_cpu)
    by_key = {k.tobytes()[:39]: s for s, k in enumerate(w.keys)}
    for rec in got[0]:
        first = w.first_map(by_key[rec["id"].tobytes()[:39]])
        assert int(rec["metrics"]["eth_protocol"]) == (0x1000 + pc.ENUM.index(first) if first else 0)


@pytest.mark.parametrize("name", ["xlat", "ring"])
def test_map_merge_device(nf, O, tab, name):
    """tab.map_merge_device on the family's widest call: maps and merged flows in device memory."""
    import torch
    fam = pc.family(name)
    call = fam.calls[-1]
    mi, mv, feats = pc.merge_maps(fam, call)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_mi, d_mv = dev(mi), dev(mv)
    d_f = {k: (dev(a), dev(b), len(a)) for k, (a, b) in feats.items()}
    total = len(mi) + sum(len(a) for a, _ in feats.values())
    d_out = {k: torch.full((total * s + 16,), 0xAB, dtype=torch.uint8, device="cuda") for k, s in SIZES.items()}
    torch.cuda.synchronize()
    rc, n, dups = tab.map_merge_device((d_mi.data_ptr(), d_mv.data_ptr(), len(mi)), {k: (i.data_ptr(), v.data_ptr(), m) for k, (i, v, m) in d_f.items()},
                                       call.n_cpu, {k: t.data_ptr() for k, t in d_out.items()}, total)
    assert rc == nf.OK and n == len(call.script) and dups == 0
    recs = d_out["records"][: n * 144].cpu().numpy().view(nf.FLOW_RECORD)
    present = d_out["present"][:n].cpu().numpy()
    parts = {k: d_out[k][: n * SIZES[k]].cpu().numpy().view(nf.ROLLUP_KINDS[k]) for k in SIZES if k not in ("records", "present")}
    check_merge(nf, O, (recs, present, parts, dups), mi, mv, feats, call.n_cpu, "%s, map merge on the device, n_cpu %d" % (name, call.n_cpu))
    for k, s in SIZES.items():
        assert (d_out[k][n * s:].cpu().numpy() == 0xAB).all(), k          # nothing behind the merged flows is touched
