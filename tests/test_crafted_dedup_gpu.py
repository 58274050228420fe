"""Kernel-dedup parity on SCRIPTED flows, on every route the mode has. The other kernel-dedup tests feed seeded streams whose
interfaces, directions and TLS fields are drawn at random: whether a given short order of events — a side interface before the
first counted record of a call, interface 0 first, one direction twice and then another, the list filling between two directions of
one interface, a window move between them — reaches a given kernel depends on the seed. tests/dedupcraft.py enumerates the orders
(four exhaustive families, two seeded ones around the capacity cut-off and the 64-lane wave); here every family goes through

    1  one call: the direct kernels (variant 1), the streaming + partition passes (10; 12 without retry rounds; 16 sorted first)
    2  one call per round (round j = the j-th record of every flow): every script meets its own slot's state at every position;
       also on a table with deferred claims (2^21 slots: grouped first flush, two-phase path afterwards)
    3  the sequence window moving (csrc/nfagg_rebase.hip k_rebase<true>) after every round in turn, after every round of one run
       (ranks of ranks), and twice with none of the flows' records in between
    4  the window's last numbers: the smallest ~seq and the largest seq + 1 a tag can hold
    5  evict on full inside the stream
    6  a sub-flow table alone (local_fold): the join of csrc/nfagg_dedup_join.hip
    7  four ranks, the rounds dealt round the ranks, folded in ascending and in descending rank order
    8  a one-process local-fold group

and the sorted eviction must equal the oracle's kernel-dedup Accounter bit for bit — which tests/test_oracle_ref.py pins to the
reference's own bpf/flows.c on exactly these families. A failure names the family, the script and the leg."""
import numpy as np
import pytest

import dedupcraft as dc
import keycraft as kc
from conftest import as_bytes, assert_records_equal
from test_dedup_gpu import check_dedup
from test_dedup_local_fold_gpu import Ranks

pytestmark = pytest.mark.gpu

MAX_ENTRIES = 1 << 15                       # the smallest table (2^16 slots) on which every route runs its real kernels
WINDOW = 0xFFFFFFF0                         # csrc/nfagg_api.hip kSeqWindow: a call of n records moves the window when used + n >= WINDOW
ROUNDS = {"intf": 5, "ssl": 5, "hello": 3, "last": 5, "capacity": 24, "wave": 64}     # the longest script of each family
CUTS = [(name, j) for name in dc.FAMILIES for j in range(1, ROUNDS[name])]


class Case:
    """A family with its layouts and the oracle's flows (one Accounter that never fills), built once per module."""

    def __init__(self, nf, O, name):
        self.nf, self.O, self.name = nf, O, name
        self.fam = fam = dc.family(name)
        assert fam.length.max() == ROUNDS[name]
        ev = O.run_accounter(fam.recs, 1 << 20, mode=1)
        assert len(ev) == 1 and len(ev[0][1]) == fam.n_scripts
        self.want = ev[0][1]
        self.rm, self.bounds = dc.round_major(fam)
        self.orders = {"flow_major": dc.flow_major(fam), "round_major": self.rm, "shuffled": dc.shuffled(fam)}
        self._stranger = self._rounds = None

    def recs(self, layout):
        return self.fam.recs[self.orders[layout]]

    def rounds(self):
        if self._rounds is None:
            r = self.fam.recs[self.rm]
            self._rounds = [r[self.bounds[j]:self.bounds[j + 1]] for j in range(len(self.bounds) - 1)]
        return self._rounds

    def fulls(self, layout, max_entries):
        """How often Accounter.Account finds the map full on this arrival order (account.go:85-94), counted on script numbers."""
        live, n = set(), 0
        for s in self.fam.script[self.orders[layout]].tolist():
            if s not in live:
                if len(live) >= max_entries:
                    live.clear()
                    n += 1
                live.add(s)
        return n

    def stranger(self):
        """One record of a flow that is in no script, and the oracle's flows with it (its position in the stream does not matter:
        it shares no slot with anybody)."""
        if self._stranger is None:
            rec = self.fam.recs[:1].copy()
            rec.view(np.uint8).reshape(1, 144)[0, :38] ^= 0xA5
            both = np.concatenate([self.fam.recs, rec])
            assert kc.distinct_flows(both) == self.fam.n_scripts + 1
            self._stranger = (rec, self.O.run_accounter(both, 1 << 20, mode=1)[0][1])
        return self._stranger

    def check(self, got, leg, want=None):
        """Bit for bit; the message names the family, the first differing flow's script and the leg."""
        want = self.want if want is None else want
        try:
            assert_records_equal(got, want, "%s, %s" % (self.name, leg))
        except AssertionError as e:
            raise AssertionError("%s\n  %s" % (e, self.blame(got, want))) from None

    def blame(self, got, want):
        g, w = as_bytes(got), as_bytes(want)
        if g.shape != w.shape:
            return "the flows differ in number"
        i = int(np.nonzero((g != w).any(axis=1))[0][0])
        try:
            return "first differing flow: " + self.fam.describe(self.fam.script_of_key(w[i, :40]))
        except KeyError:
            return "first differing flow is in no script"


@pytest.fixture(scope="module")
def lab(nf, O):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(nf, O, name)
        return cache[name]
    return get


def table(nf, **kw):
    kw.setdefault("max_entries", MAX_ENTRIES)
    return nf.FlowTable(mode=nf.MODE_KERNEL_DEDUP, **kw)


def feed(nf, tab, recs):
    assert tab.ingest(recs.view(nf.FLOW_RECORD)) == (nf.OK, len(recs))


def evicted(nf, tab):
    n_live = len(tab)
    got = nf.sort_by_key(tab.evict(nf.REASON_CLOSING))
    assert len(got) == n_live
    return got


# ---------------------------------------------------------------- 1: one call
@pytest.mark.parametrize("layout", ["flow_major", "round_major"])
@pytest.mark.parametrize("ingest_variant", [1, 10, 12, 16])
@pytest.mark.parametrize("family", dc.FAMILIES)
def test_one_call(nf, lab, family, ingest_variant, layout):
    """Variant 1: k_dedup_claim / k_dedup_fold. The others: the streaming pass and the partition pass — a family's sub-flows
    outnumber a workgroup's 1 024 cache entries, so cached and spilled records of one flow meet; flow-major, a wave holds whole
    flows (all 64 records of one, in `wave`)."""
    c = lab(family)
    with table(nf, ingest_variant=ingest_variant) as tab:
        feed(nf, tab, c.recs(layout))
        c.check(evicted(nf, tab), "one call, variant %d, %s" % (ingest_variant, layout))


# ---------------------------------------------------------------- 2: round by round
@pytest.mark.parametrize("ingest_variant,log2_slots", [(1, 0), (10, 0), (10, 21), (16, 21)])
@pytest.mark.parametrize("family", dc.FAMILIES)
def test_round_by_round(nf, lab, family, ingest_variant, log2_slots):
    """One call per round: record j of every script finds the slot as records 0..j-1 left it, on every route. 2^21 slots: the
    partition pass claims per workgroup — round 1 takes the grouped first flush, the later rounds the two-phase path."""
    c = lab(family)
    kw = dict(table_log2_slots=log2_slots) if log2_slots else {}
    with table(nf, ingest_variant=ingest_variant, **kw) as tab:
        for r in c.rounds():
            feed(nf, tab, r)
        c.check(evicted(nf, tab), "round by round, variant %d, log2 slots %d" % (ingest_variant, log2_slots))


# ---------------------------------------------------------------- 3: the window moves
class Window:
    """A table fed call by call with the position leaping on demand. `used` restates csrc/nfagg_api.hip ensure_seq_window: the
    window-relative position, which a move sets back to kRebaseKeep."""

    def __init__(self, nf, tab):
        self.nf, self.tab = nf, tab
        self.keep = kc._grab("nfagg_rebase.hip", r"^constexpr uint32_t kRebaseKeep = (\d+);")
        self.used = self.records = self.skipped = self.moves = 0

    def skip(self, s):
        assert s >= 0
        self.tab.debug_skip_sequence(s)
        self.used += s
        self.skipped += s

    def leap_for(self, n):
        """The smallest leap after which a call of n records does not fit any more: used + n == WINDOW."""
        self.skip(WINDOW - self.used - n)

    def feed(self, recs, moves):
        """One call; the window must move exactly `moves` (0 or 1) times at it."""
        n = len(recs)
        assert (self.used + n >= WINDOW) == bool(moves), "the rule says otherwise"
        feed(self.nf, self.tab, recs)
        self.used = (self.keep if moves else self.used) + n
        self.records += n
        self.moves += moves
        st = self.tab.stats()
        assert st.sequence_rebases == self.moves, "sequence_rebases %d, expected %d" % (st.sequence_rebases, self.moves)
        assert st.epoch_seq == self.records + self.skipped


@pytest.mark.parametrize("ingest_variant", [1, 10])
@pytest.mark.parametrize("family,cut", CUTS, ids=["%s-cut%d" % fc for fc in CUTS])
def test_window_moves_at_one_cut(nf, lab, family, cut, ingest_variant):
    """Between rounds `cut` and `cut + 1` the position leaps so that the next call no longer fits: the (up to 21) sequence numbers
    of every slot become their ranks between record `cut` and record `cut + 1` of every script — between two directions of one
    interface, between the side interface and the record that would have filled the list, before the counted record, ..."""
    c = lab(family)
    with table(nf, ingest_variant=ingest_variant) as tab:
        w = Window(nf, tab)
        for j, r in enumerate(c.rounds(), 1):
            w.feed(r, 1 if j == cut + 1 else 0)
            if j == cut:
                w.leap_for(len(c.rounds()[j]))
        assert w.moves == 1
        c.check(evicted(nf, tab), "window moved after round %d, variant %d" % (cut, ingest_variant))


@pytest.mark.parametrize("ingest_variant", [1, 10])
@pytest.mark.parametrize("family", dc.FAMILIES)
def test_window_moves_at_every_cut(nf, lab, family, ingest_variant):
    """A move before every call but the first: ranks of ranks, the numbers below kRebaseKeep used again and again."""
    c = lab(family)
    rounds = c.rounds()
    with table(nf, ingest_variant=ingest_variant) as tab:
        w = Window(nf, tab)
        for j, r in enumerate(rounds):
            if j:
                w.leap_for(len(r))
            w.feed(r, 1 if j else 0)
        assert w.moves == len(rounds) - 1
        c.check(evicted(nf, tab), "window moved at every cut, variant %d" % ingest_variant)


@pytest.mark.parametrize("ingest_variant", [1, 10])
@pytest.mark.parametrize("family", dc.FAMILIES)
def test_window_moves_twice_with_no_record_of_the_flows_between(nf, lab, family, ingest_variant):
    """A move only ever happens at a call, and a call has records: the call between the two moves holds ONE record of a flow that
    is in no script — every script's slot is ranked twice with nothing folded into it in between."""
    c = lab(family)
    rounds = c.rounds()
    cut = len(rounds) // 2
    rec, want = c.stranger()
    with table(nf, ingest_variant=ingest_variant) as tab:
        w = Window(nf, tab)
        for j, r in enumerate(rounds):
            if j == cut:
                w.leap_for(1)
                w.feed(rec, 1)
                w.leap_for(len(r))
            w.feed(r, 1 if j == cut else 0)
        assert w.moves == 2
        c.check(evicted(nf, tab), "two moves after round %d, variant %d" % (cut, ingest_variant), want)


# ---------------------------------------------------------------- 4: the window's last numbers
@pytest.mark.parametrize("one_more", [False, True], ids=["fits", "one_more"])
@pytest.mark.parametrize("ingest_variant", [1, 10])
@pytest.mark.parametrize("family", ["intf", "last"])
def test_the_last_numbers_of_the_window(nf, lab, family, ingest_variant, one_more):
    """The rule admits a call of n records while used + n < WINDOW: its last record then takes the relative number WINDOW - 2 at
    most — the smallest ~seq of a "first" tag, the largest seq + 1 of a "last" tag, in both halves of `end`. The call that starts
    at the same position with one record more (the record before it) must move the window instead."""
    c = lab(family)
    recs = c.recs("round_major")
    p = int(c.bounds[len(c.bounds) // 2])
    n = len(recs) - p
    with table(nf, ingest_variant=ingest_variant) as tab:
        w = Window(nf, tab)
        if one_more:
            w.feed(recs[:p - 1], 0)
            w.skip(WINDOW - 1 - len(recs) + 1)               # the call starts where it does below, and has n + 1 records
            assert w.used + n + 1 == WINDOW
            w.feed(recs[p - 1:], 1)
        else:
            w.feed(recs[:p], 0)
            w.skip(WINDOW - 1 - len(recs))                   # used + n == WINDOW - 1: the last record is number WINDOW - 2
            assert w.used + n - 1 == WINDOW - 2
            w.feed(recs[p:], 0)
        assert w.moves == int(one_more)
        c.check(evicted(nf, tab), "last numbers of the window, variant %d, %s" % (ingest_variant, "one more" if one_more else "fits"))


# ---------------------------------------------------------------- 5: evict on full inside the stream
# Families with too few flows for two evictions on full at a size (64 in `wave`, 1 884 in `hello`): the count the inputs give.
FEWER_FULLS = {("wave", 999, "flow_major"): 0, ("wave", 999, "round_major"): 0, ("wave", 50, "flow_major"): 1, ("hello", 999, "flow_major"): 1}


@pytest.mark.parametrize("ingest_variant", [0, 10])
@pytest.mark.parametrize("layout", ["flow_major", "round_major"])
@pytest.mark.parametrize("max_entries", [50, 999])
@pytest.mark.parametrize("family", dc.FAMILIES)
def test_evict_on_full_inside_the_stream(nf, O, lab, family, max_entries, layout, ingest_variant):
    """Batches of 4 096: the whole eviction sequence, every eviction bit for bit. Round-major, a flow is cut at any position of
    its script and its next record starts a NEW flow (another first interface, another first record's list)."""
    c = lab(family)
    try:
        want = check_dedup(nf, O, c.recs(layout), max_entries, 4096, ingest_variant=ingest_variant)
    except AssertionError as e:
        raise AssertionError("%s, evict on full at %d, %s, variant %d: %s" % (family, max_entries, layout, ingest_variant, e)) from None
    fulls = sum(1 for r, _ in want if r == "full")
    assert fulls == c.fulls(layout, max_entries)
    assert fulls >= 2 or fulls == FEWER_FULLS[family, max_entries, layout]


# ---------------------------------------------------------------- 6: a sub-flow table alone
@pytest.mark.parametrize("by_round", [False, True], ids=["one_call", "round_by_round"])
@pytest.mark.parametrize("ingest_variant", [1, 10])
@pytest.mark.parametrize("family", dc.FAMILIES)
def test_subflow_table_alone(nf, lab, family, ingest_variant, by_round):
    """local_fold: one slot per (flow, interface), each holding both roles of its interface; the eviction joins them — F is the
    interface of the sub-flow with the smallest first sequence number. Against the flow-keyed oracle."""
    c = lab(family)
    with table(nf, ingest_variant=ingest_variant, local_fold=True) as tab:
        for r in (c.rounds() if by_round else [c.recs("flow_major")]):
            feed(nf, tab, r)
        got = nf.sort_by_key(tab.evict(nf.REASON_CLOSING))
        c.check(got, "sub-flow table, variant %d, %s" % (ingest_variant, "round by round" if by_round else "one call"))


# ---------------------------------------------------------------- 7: four ranks
@pytest.mark.parametrize("family", dc.FAMILIES)
def test_four_ranks_fold_the_rounds_in_turn(nf, lab, family):
    """Round j goes to rank j % 4 with the sequence numbers [j N, j N + its records): consecutive records of every flow lie on
    different ranks. Epoch 1: the ranks fold in ascending order. Epoch 2: in descending order — rank 0, which holds every flow's
    first record, folds last, so F is decided by a record folded after all the others. Then the tick: export, merge, join."""
    c = lab(family)
    rounds, N = c.rounds(), len(c.fam.recs)
    R = Ranks(nf, 4, max_entries=1 << 16)
    try:
        for epoch, order in enumerate(([0, 1, 2, 3], [3, 2, 1, 0])):
            for rank in order:
                for j in range(rank, len(rounds), 4):
                    R.fold(rank, rounds[j], j * N)
            got, _ = R.tick()
            c.check(got, "four ranks, folding in rank order %s" % order)
    finally:
        R.close()


# ---------------------------------------------------------------- 8: a one-process group
@pytest.mark.parametrize("family", dc.FAMILIES)
def test_local_fold_group(nf, lab, family):
    """FlowGroup([0] * 4, local_fold=True): the chunks of the shuffled stream go round the members, every flow's records — and
    interfaces — are spread over them, the eviction brings the sub-flows to their owners and joins them."""
    c = lab(family)
    recs = c.recs("shuffled")
    staging = 1_000 if len(recs) < 8_000 else 7_000
    with nf.FlowGroup([0] * 4, max_entries=1 << 16, local_fold=True, mode=nf.MODE_KERNEL_DEDUP, staging_records=staging) as grp:
        assert grp.ingest(recs.view(nf.FLOW_RECORD)) == (nf.OK, len(recs))
        assert all(m.stats().records_ingested > 0 for m in grp.members)
        got = nf.sort_by_key(grp.evict(nf.REASON_TIMEOUT))
    c.check(got, "local-fold group")
