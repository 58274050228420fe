"""Sketch parity on CRAFTED address hashes. The other sketch tests feed 20 000 - 30 000 addresses with effectively random hashes:
no HyperLogLog register rises above about 8, registers 0 and m - 1 and the largest rho (where only the sentinel bit ends the count)
are never reached, the four registers of one word are never raised against each other, and the configuration's own limits
(hll_p 4 and 18, cm_depth 1 and 8, cm_log2_width 4) are never used. tests/sketchcraft.py plants families of addresses with chosen
hashes (see there) into a seeded stream; here the stream goes through every route that updates the sketches — the sketch kernel of
its own, the fused updates of the cached kernels, the two-pass fold, the kernel-dedup passes and the three forms of nfagg_account —
and all four snapshots must equal the oracle's, bit for bit, with the evictions and a Count-Min query of each counter family.
Every family's precondition is asserted on the oracle's arrays (sketchcraft.check_preconditions)."""
import numpy as np
import pytest

import sketchcraft as sc
from conftest import assert_records_equal
from test_account_gpu import _check as check_account
from test_crafted_sketches_cpu import check_estimate

pytestmark = pytest.mark.gpu

WHICH = ("CM_SRC", "CM_DST", "HLL_SRC", "HLL_DST")


@pytest.fixture(scope="module")
def planted(O):
    """Per configuration (records, info, the oracle's four arrays): sketchcraft's one set of streams; preconditions checked here."""
    out = sc.planted_streams(O)
    for p, depth, log2w in sc.CONFIGS:
        sc.check_preconditions(O, p, log2w, out[p][2], out[p][1])
    return out


def check_sketches(nf, O, tab, p, depth, log2w, info, sk, what):
    for name, want in zip(WHICH, sk):
        got = tab.sketch_snapshot(getattr(nf, name))
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "%s, %s: %d entries differ, first at %d: got %d want %d" % (what, name, len(bad), bad[0], got[bad[0]], want[bad[0]])
    for side, fam, which in ((0, "cm_first", nf.CM_SRC), (1, "cm_last", nf.CM_DST)):
        ip = info[fam][7].tobytes()
        cm = np.ascontiguousarray(sk[side])
        assert tab.cm_query(which, ip) == O.lib().orc_cm_query(cm.ctypes.data, depth, log2w, ip), (what, fam)
    for regs, which in ((sk[2], nf.HLL_SRC), (sk[3], nf.HLL_DST)):                       # one arithmetic in the library and the oracle
        assert tab.hll_estimate(which) == O.hll_estimate(regs, p), what


ROUTES = ["ingest 1", "ingest 7", "ingest 10", "dedup 10", "account", "account 20000", "account 30"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("p,depth,log2w", sc.CONFIGS)
def test_sketch_parity_on_crafted_addresses(nf, O, planted, p, depth, log2w, route):
    """ingest 1: the direct kernel and the sketch kernel of its own (wave-combined byte sums); 7: the single-pass cached kernel;
    10: the two-pass fold — both feed the sketches from their cache entries; dedup 10: the kernel-dedup passes (the sketches count
    every record, whatever the merge counts); account: nfagg_account with max_entries 5 000 in one call, in calls of 20 000
    records, and through the kernel chain (ingest_variant 30)."""
    recs, info, sk = planted[p]
    kind, _, arg = route.partition(" ")
    kw = dict(sketches=nf.SKETCH_CM | nf.SKETCH_HLL, cm_depth=depth, cm_log2_width=log2w, hll_p=p)
    what = "%s, p %d, depth %d, log2w %d" % (route, p, depth, log2w)
    if kind == "account":
        variant, batch = (30, len(recs)) if arg == "30" else (0, int(arg or len(recs)))
        with nf.FlowTable(max_entries=5000, ingest_variant=variant, **kw) as tab:
            check_account(nf, O, tab, recs, 5000, [batch] * (len(recs) // batch + 1))
            check_sketches(nf, O, tab, p, depth, log2w, info, sk, what)
        return
    mode = nf.MODE_KERNEL_DEDUP if kind == "dedup" else nf.MODE_ACCOUNTER
    want = O.run_accounter(recs, 1 << 20, 1 if kind == "dedup" else 0)
    assert len(want) == 1 and len(want[0][1]) == info["flows"]
    with nf.FlowTable(max_entries=1 << 15, mode=mode, ingest_variant=int(arg), **kw) as tab:
        assert tab.ingest(recs.view(nf.FLOW_RECORD)) == (nf.OK, len(recs))
        check_sketches(nf, O, tab, p, depth, log2w, info, sk, what)
        got = nf.sort_by_key(tab.evict(nf.REASON_CLOSING))
    assert_records_equal(got, want[0][1], what)


def test_half_half_registers_and_estimate(nf, O):
    """2^18 flows, p = 18: 2^17 registers at 1 and 2^17 at 47, the layout on which the oracle's estimate was 92 ULP from the exact
    value while it added its sum up in doubles. Registers bit for bit; the estimate within 2 ULP of exact arithmetic and equal to
    the oracle's."""
    recs = sc.half_half_stream(O)
    want = O.run_accounter(recs, 1 << 19)
    assert len(want) == 1 and len(want[0][1]) == len(recs)
    with nf.FlowTable(max_entries=1 << 19, sketches=nf.SKETCH_HLL, hll_p=18) as tab:
        assert tab.ingest(recs.view(nf.FLOW_RECORD)) == (nf.OK, len(recs))
        regs = tab.sketch_snapshot(nf.HLL_SRC)
        est = tab.hll_estimate(nf.HLL_SRC)
        got = nf.sort_by_key(tab.evict(nf.REASON_CLOSING))
    assert np.array_equal(regs, sc.half_half_registers()) and np.array_equal(regs, O.sketches(recs, 1, 4, 18)[2])
    exact, lib, orc = check_estimate(nf, O, "half_half", 18, regs)
    assert est == lib == orc and sc.ulps(est, exact) <= 2
    assert_records_equal(got, want[0][1], "half_half")
