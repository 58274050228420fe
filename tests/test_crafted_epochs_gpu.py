"""nfagg_account on CRAFTED calls (tests/epochcraft.py): the evict-on-full loop with its epochs found first
(csrc/nfagg_epoch_par.hip, csrc/nfagg_api_account.hip) and its fallback, the kernel chain (csrc/nfagg_epoch_chain.hip,
ingest_variant 30), driven to the places where their designs have edges. The seeded Zipf streams of tests/test_account_par_gpu.py
leave to chance where a cut falls inside a block, a wave, a row or a group of four records of the cut walk, how long a flow's
segment is relative to kSegShort, kSegHuge and kHugeChunk, and which record of a 5 000-record segment carries the only non-zero DSCP.

    cuts_*     cuts at chosen record indices: every residue mod 4, both sides of a row (256), a wave (1 024), a block (16 384) and
               the fifth block (65 536), four consecutive cuts in one group of four, an epoch from a block's last group to the next
               block's first, two blocks without a new flow, a cut at the last record, calls of exactly one block / one block + 1 /
               four blocks, a planned call delivered two evictions at a time (NFAGG_TRUNCATED, the next call starts at a cut)
    live_*     a first nfagg_ingest leaves flows in the table (k_par_live, the first epoch's budget): a full table and a new
               flow at record 0, a full table and live flows first, a partly filled one, a one-home family half live and half
               new, the marker hashes 0, 1, 2, 2^64 - 1 live and new, one 64-bit hash live and new
    seg_*      one middle epoch per segment length on both sides of every threshold, by records and by sorted positions (a second
               flow with the same key hash interleaved), a collider's head inside the hot flow's run, the sketches fed per segment
    field_*    the hot flow's order-dependent fields zero but on one or two chosen records of a short, a long and a huge segment;
               the 64-bit end whose high half decides; start on one record only; an all-zero head

Every call is checked on the CPU first (tests/test_epochcraft_cpu.py: cuts, the oracle's evictions, segment classes, the
deciding records). Here every eviction must be bit-identical, in order, to the oracle's Accounter — on the default path
(account_epochs_first >= 1, nothing declined, no chain) and on the chain (ingest_variant 30)."""
import numpy as np
import pytest

import epochcraft as ec
from conftest import assert_records_equal
from test_account_gpu import _check

pytestmark = pytest.mark.gpu

NAMES = list(ec.cases())
_WANT = {}


def oracle_evictions(O, name):
    """The oracle's evictions of a case, computed once and left unchanged."""
    if name not in _WANT:
        call = ec.get(O, name)
        _WANT[name] = O.run_accounter(call.everything(), call.max_entries)
    return _WANT[name]


class Recording:
    """A FlowTable as test_account_gpu._check drives it, keeping what it delivered."""

    def __init__(self, tab):
        self.tab, self.epochs, self.closing = tab, [], None

    def account(self, records, **kw):
        rc, c, epochs = self.tab.account(records, **kw)
        self.epochs += [e.copy() for e in epochs]
        return rc, c, epochs

    def evict(self, reason):
        self.closing = self.tab.evict(reason)
        return self.closing


def drive(nf, O, name, tab, after_ingest=None):
    """The case's calls through tab; every eviction against the oracle's. Returns the evictions on full as delivered.
    after_ingest(tab): called between the first call (nfagg_ingest of the live flows) and the account call."""
    call = ec.get(O, name)
    M, view = call.max_entries, call.recs.view(nf.FLOW_RECORD)
    want = oracle_evictions(O, name)
    rec = Recording(tab)
    if call.live_recs is None and call.deliver is None:
        assert _check(nf, O, rec, call.recs, M, [len(call.recs)]) == len(want)
        return rec.epochs
    if call.live_recs is not None:                                    # the table's flows come from a first nfagg_ingest
        assert tab.ingest(call.live_recs.view(nf.FLOW_RECORD)) == (nf.OK, len(call.live_recs))
        assert len(tab) == call.live0
        if after_ingest:
            after_ingest(tab)
    kw = dict(out_cap=call.deliver[0], max_epochs=call.deliver[1]) if call.deliver else {}
    off = 0
    while off < len(view):
        rc, c, epochs = rec.account(view[off:], **kw)
        assert rc in (nf.OK, nf.TRUNCATED) and c > 0
        if call.deliver:                                              # the walk stopped at max_cuts: the next call starts at a cut
            assert len(epochs) <= call.deliver[0] // M and (rc == nf.TRUNCATED or off + c == len(view))
            assert off + c == len(view) or off + c in call.cuts
        off += c
    got = [("full", nf.sort_by_key(e)) for e in rec.epochs] + [("closing", nf.sort_by_key(rec.evict(nf.REASON_CLOSING)))]
    assert [r for r, _ in got] == [r for r, _ in want], (len(got), len(want))
    for k, ((_, g), (_, w)) in enumerate(zip(got, want)):
        assert_records_equal(g, w, "%s: eviction %d of %d" % (name, k, len(want)))
    return rec.epochs


def check_path(nf, name, st, variant):
    print("%s variant %d: account_epochs_first %d, account_declined %d, account_chain %d" %
          (name, variant, st.account_epochs_first, st.account_declined, st.account_chain))
    if variant == 0:
        assert st.account_epochs_first >= 1 and st.account_declined == 0 and st.account_chain == 0
    else:
        assert st.account_epochs_first == 0 and st.account_chain >= 1


def find_flow(O, ev, key):
    """The evicted record of the flow with this key, in the oracle's field names."""
    ev = np.ascontiguousarray(ev).view(O.FLOW_RECORD)
    raw = ev.view(np.uint8).reshape(len(ev), 144)
    hit = np.nonzero((raw[:, :39] == key[:39]).all(axis=1))[0]
    assert len(hit) == 1
    return ev[hit[0]]


@pytest.mark.parametrize("variant", [0, 30])
@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("cuts_")])
def test_cuts_at_chosen_records(nf, O, name, variant):
    call = ec.get(O, name)
    with nf.FlowTable(max_entries=call.max_entries, ingest_variant=variant) as tab:
        epochs = drive(nf, O, name, tab)
        st = tab.stats()
    assert len(epochs) == len(call.cuts)
    assert st.records_ingested == len(call.recs) and st.evictions[nf.REASON_FULL] == len(call.cuts)
    check_path(nf, name, st, variant)
    if call.deliver and variant == 0:                                 # every resumed call was long enough for the default path again
        assert st.account_epochs_first == -(-len(call.cuts) // (call.deliver[0] // call.max_entries)) + 1


@pytest.mark.parametrize("variant", [0, 30])
@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("live_")])
def test_a_live_table_and_the_first_epochs_budget(nf, O, name, variant):
    call = ec.get(O, name)
    with nf.FlowTable(max_entries=call.max_entries, ingest_variant=variant) as tab:
        def one_home(tab):
            # half of the family is live and fills the chain from the table's last slot round to slot K / 2 - 2: the furthest of
            # them has walked past the others; a new one of the family walks past all of them to a free slot and comes out new
            st1 = tab.stats()
            mask = int(st1.table_slots) - 1
            print("%s variant %d: %d slots, max_probe %d after the first call (precondition: >= %d)" %
                  (name, variant, mask + 1, st1.max_probe, ec.ONE_HOME_K // 2 - 1))
            assert mask & ec.ONE_HOME_LOW == mask, "the family's home slot is meant to be this table's last"
            assert st1.max_probe >= ec.ONE_HOME_K // 2 - 1

        epochs = drive(nf, O, name, tab, one_home if name == "live_one_home" else None)
        st = tab.stats()
    assert len(epochs) == len(call.cuts)
    check_path(nf, name, st, variant)


@pytest.mark.parametrize("variant", [0, 30])
@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("seg_")])
def test_segments_on_both_sides_of_every_threshold(nf, O, name, variant):
    call = ec.get(O, name)
    kw = dict(sketches=nf.SKETCH_CM | nf.SKETCH_HLL, cm_log2_width=12, hll_p=8) if call.info.get("sketch") else {}
    with nf.FlowTable(max_entries=call.max_entries, ingest_variant=variant, **kw) as tab:
        epochs = drive(nf, O, name, tab)
        st = tab.stats()
        if kw:                                                        # a segment feeds the sketches once, with its byte sum
            cs, cd, hs, hd = O.sketches(call.recs, 4, 12, 8)
            assert np.array_equal(tab.sketch_snapshot(nf.CM_SRC), cs) and np.array_equal(tab.sketch_snapshot(nf.CM_DST), cd)
            assert np.array_equal(tab.sketch_snapshot(nf.HLL_SRC), hs) and np.array_equal(tab.sketch_snapshot(nf.HLL_DST), hd)
    check_path(nf, name, st, variant)
    for seg in call.info["segments"]:                                 # the hot flow's eviction holds exactly its L records
        got = find_flow(O, epochs[seg["epoch"]], call.keys[seg["hot"]])
        idx = np.nonzero(call.flow == seg["hot"])[0]
        m = call.recs["metrics"]
        assert len(idx) == seg["L"] and int(got["metrics"]["packets"]) == sum(int(x) for x in m["packets"][idx]) & 0xFFFFFFFF      # (Go's uint32 wraps)
        assert int(got["metrics"]["bytes"]) == sum(int(x) for x in m["bytes"][idx]) & ec.M64


@pytest.mark.parametrize("variant", [0, 30])
@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("field_")])
def test_the_record_that_decides_a_field(nf, O, name, variant):
    call = ec.get(O, name)
    with nf.FlowTable(max_entries=call.max_entries, ingest_variant=variant) as tab:
        epochs = drive(nf, O, name, tab)
        st = tab.stats()
    check_path(nf, name, st, variant)
    for seg in call.info["segments"]:                                 # beside the oracle: the DESIGNED record's value, last or first as the field's rule says
        got = ec.fields_of(find_flow(O, epochs[seg["epoch"]], call.keys[seg["hot"]]))
        for field, v in seg["expect"].items():
            assert got[field] == v, "%s epoch %d (%s, records %s): %s" % (name, seg["epoch"], seg["kind"], seg["nz"], field)
