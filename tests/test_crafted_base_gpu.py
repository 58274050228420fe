"""AccumulateBase parity on SCRIPTED flows, on every route accounter mode has. The other accounter-mode fold tests take their
records from the oracle's stream generator, whose start and end grow with the arrival position and stay below 2^21, whose tagged
fields never carry all-ones and whose MAC halves are never zero: a kernel that kept the last end, the first non-zero start or only
the low halves would pass them. tests/basecraft.py enumerates the orders of values that tell each rule of
pkg/model/flow_content.go:28-61 from its neighbours (four exhaustive families, two seeded ones: the 64-lane wave and the hot cache
entry); here every family goes through

    1  one call: the direct kernel (variant 1), the single-pass cached kernels (3, 7), the two-pass fold (10; 11 without its
       admission filter; 17 with the pass 1 that publishes its entries) and the default by size (0), in three arrival orders
    2  one call per round (round j = the j-th record of every flow): every script meets its own slot's state at every position;
       also on a table with deferred claims (2^21 slots)
    3  the sequence window moving (csrc/nfagg_rebase.hip k_rebase<false>) after every round in turn, after every round of one run,
       and twice with none of the flows' records in between
    4  the window's last numbers: the largest seq + 1 above sampling = 0xFFFFFFFF - pos, the smallest ~seq on the MAC and
       first-record tags
    5  evict on full inside the stream
    6  nfagg_account: epochs found first, and the kernel chain (variant 30)
    7  ranks: the rounds dealt round four ranks and folded in ascending and descending rank order, three ranks with contiguous
       slices, four ranks restarting their window together
    8  a one-process local-fold group of 2 and of 3 members

and the sorted eviction must equal the oracle's Accounter bit for bit — which tests/test_basecraft_cpu.py holds against a
restatement of the Go text in Python integers on exactly these families. A failure names the family, the script and the leg.

`hot` has 4 096 rounds of eight records: where a leg goes round by round, its rounds are blocks of 64 positions (512 records)."""
import os
import re

import numpy as np
import pytest

import basecraft as bc
import keycraft as kc
from conftest import as_bytes, assert_records_equal
from test_account_gpu import _check as check_account
from test_parity_gpu import check_against_oracle
from test_partials_gpu import Ranks

pytestmark = pytest.mark.gpu

MAX_ENTRIES = 1 << 15                       # the smallest table (2^16 slots) on which every route runs its real kernels
LAYOUTS = ("flow_major", "round_major", "shuffled")
HOT_BLOCK = 64
ROUNDS = {"times": 4, "lastnz": 4, "macs": 3, "sums": 3, "wave": 64, "hot": bc.HOT_LEN // HOT_BLOCK}
CUTS = [(name, j) for name in bc.FAMILIES for j in range(1, ROUNDS[name])]
DOOR_VARIANTS = (10, 17)                    # pass 1 admits a flow to its cache on the flow's SECOND record in the workgroup's share


def seq_window():
    """csrc/nfagg_api.hip kSeqWindow: a call of n records moves the window when used + n >= kSeqWindow."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "netobserv-ebpf-agent_amd", "csrc", "nfagg_api.hip")
    with open(path) as f:
        m = re.search(r"^constexpr uint64_t kSeqWindow = (0x[0-9A-Fa-f]+)ull;", f.read(), re.M)
    assert m, "kSeqWindow"
    return int(m.group(1), 16)


WINDOW = seq_window()


class Case:
    """A family with its layouts and the oracle's flows (one Accounter that never fills), built once per module."""

    def __init__(self, nf, O, name):
        self.nf, self.O, self.name = nf, O, name
        self.fam = fam = bc.family(name)
        self.want = self.oracle(fam.recs)
        assert len(self.want) == fam.n_scripts
        if name == "hot":                   # rounds of 64 positions
            self.rm = np.lexsort((fam.pos, fam.script, fam.pos // HOT_BLOCK))
            self.bounds = np.concatenate([[0], np.cumsum(np.bincount(fam.pos // HOT_BLOCK))])
        else:
            self.rm, self.bounds = bc.round_major(fam)
        assert len(self.bounds) - 1 == ROUNDS[name]
        self.orders = {"flow_major": bc.flow_major(fam), "round_major": self.rm, "shuffled": bc.shuffled(fam)}
        self._stranger = self._rounds = None

    def oracle(self, recs):
        ev = self.O.run_accounter(recs, 1 << 20, 0)
        assert len(ev) == 1
        return ev[0][1]

    def recs(self, layout):
        return self.fam.recs[self.orders[layout]]

    def rounds(self):
        if self._rounds is None:
            r = self.fam.recs[self.rm]
            self._rounds = [r[self.bounds[j]:self.bounds[j + 1]] for j in range(len(self.bounds) - 1)]
        return self._rounds

    def stranger(self):
        """One record of a flow that is in no script, and the oracle's flows with it."""
        if self._stranger is None:
            rec = self.fam.recs[:1].copy()
            rec.view(np.uint8).reshape(1, 144)[0, :38] ^= 0xA5
            both = np.concatenate([self.fam.recs, rec])
            assert kc.distinct_flows(both) == self.fam.n_scripts + 1
            self._stranger = (rec, self.oracle(both))
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
    return nf.FlowTable(**kw)


def feed(nf, tab, recs):
    assert tab.ingest(recs.view(nf.FLOW_RECORD)) == (nf.OK, len(recs))


def evicted(nf, tab):
    n_live = len(tab)
    got = nf.sort_by_key(tab.evict(nf.REASON_CLOSING))
    assert len(got) == n_live
    return got


# ---------------------------------------------------------------- 1: one call
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ingest_variant", [0, 1, 3, 7, 10, 11, 17])
@pytest.mark.parametrize("family", bc.FAMILIES)
def test_one_call(nf, lab, family, ingest_variant, layout):
    """k_ingest_direct (1; 0 for the families below 6 144 records), k_ingest_cached (3, 7; 0 above), k_pass1 / k_pass1_free and
    k_pass2 (10, 11, 17). Flow-major, a wave holds whole flows (all 64 records of one, in `wave`) and every lane of it hits one
    cache entry or one slot; round-major, the records of a flow lie in different tiles.

    Precondition of the two-pass legs with the admission filter (10, 17): records_bypassed > 0. A pass-1 workgroup admits a flow to
    its cache on the flow's second record in its share, so the first is spilled to pass 2 whatever the layout: cached and spilled
    records of one flow meet in pass 2's entry, and with them a start or end that is smaller than the one before."""
    c = lab(family)
    what = "one call, variant %d, %s" % (ingest_variant, layout)
    with table(nf, ingest_variant=ingest_variant) as tab:
        feed(nf, tab, c.recs(layout))
        st = tab.stats()
        print("%s, %s: records_bypassed %d of %d, max_probe %d" % (family, what, st.records_bypassed, st.records_ingested, st.max_probe))
        assert st.records_ingested == len(c.fam.recs)
        if ingest_variant in DOOR_VARIANTS:
            assert st.records_bypassed > 0, "no record was spilled to pass 2"
        c.check(evicted(nf, tab), what)


# ---------------------------------------------------------------- 2: round by round
@pytest.mark.parametrize("ingest_variant,log2_slots", [(1, 0), (7, 0), (10, 0), (10, 21), (17, 21)])
@pytest.mark.parametrize("family", bc.FAMILIES)
def test_round_by_round(nf, lab, family, ingest_variant, log2_slots):
    """One call per round: record j of every script finds the slot as records 0..j-1 left it — probe_home's hints and the atomics
    merge_partial skips on them, merge_partial_exclusive's read-modify-write. 2^21 slots: pass 2 claims per workgroup."""
    c = lab(family)
    kw = dict(table_log2_slots=log2_slots) if log2_slots else {}
    with table(nf, ingest_variant=ingest_variant, **kw) as tab:
        for r in c.rounds():
            feed(nf, tab, r)
        st = tab.stats()
        print("%s, round by round, variant %d, log2 slots %d: records_bypassed %d" % (family, ingest_variant, log2_slots, st.records_bypassed))
        if ingest_variant in DOOR_VARIANTS:
            assert st.records_bypassed > 0, "no record was spilled to pass 2"
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
    """Between rounds `cut` and `cut + 1` the position leaps so that the next call no longer fits: the sequence numbers of every
    slot become their ranks between record `cut` and record `cut + 1` of every script — between the record that set sampling and
    the one that sets it again, between two non-zero MACs, ..."""
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
@pytest.mark.parametrize("family", bc.FAMILIES)
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
        print("%s, variant %d: sequence_rebases %d" % (family, ingest_variant, tab.stats().sequence_rebases))
        c.check(evicted(nf, tab), "window moved at every cut, variant %d" % ingest_variant)


@pytest.mark.parametrize("ingest_variant", [1, 10])
@pytest.mark.parametrize("family", bc.FAMILIES)
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
@pytest.mark.parametrize("how", ["whole", "fits", "one_more"])
@pytest.mark.parametrize("ingest_variant", [1, 7, 10])
@pytest.mark.parametrize("family", bc.FAMILIES)
def test_the_last_numbers_of_the_window(nf, lab, family, ingest_variant, how):
    """The rule admits a call of n records while used + n < WINDOW: its last record then takes the relative number WINDOW - 2 —
    the largest seq + 1 a "last non-zero" tag can hold (above sampling = 0xFFFFFFFF - pos in lastnz: a tag word of all ones but a
    few bits), the smallest ~seq of a MAC or first-record tag. whole: the family's one call ends there. fits: the second half of
    its rounds does. one_more: the call that starts at the same position with one record more must move the window instead."""
    c = lab(family)
    recs = c.recs("round_major")
    p = 0 if how == "whole" else int(c.bounds[len(c.bounds) // 2])
    n = len(recs) - p
    with table(nf, ingest_variant=ingest_variant) as tab:
        w = Window(nf, tab)
        if how == "one_more":
            w.feed(recs[:p - 1], 0)
            w.skip(WINDOW - 1 - len(recs) + 1)               # the call starts where it does below, and has n + 1 records
            assert w.used + n + 1 == WINDOW
            w.feed(recs[p - 1:], 1)
        else:
            if p:
                w.feed(recs[:p], 0)
            w.skip(WINDOW - 1 - len(recs))                   # used + n == WINDOW - 1: the last record is number WINDOW - 2
            assert w.used + n - 1 == WINDOW - 2
            w.feed(recs[p:], 0)
        assert w.moves == int(how == "one_more")
        c.check(evicted(nf, tab), "last numbers of the window, variant %d, %s" % (ingest_variant, how))


# ---------------------------------------------------------------- 5: evict on full inside the stream
FULL_FAMILIES = [f for f in bc.FAMILIES if f != "hot"]      # eight flows never fill a table of 50, and two full evictions of 2 prove little


@pytest.mark.parametrize("ingest_variant", [0, 10])
@pytest.mark.parametrize("batch", [4096, 1 << 30])
@pytest.mark.parametrize("layout", ["round_major", "shuffled"])
@pytest.mark.parametrize("small", [True, False], ids=["50", "third"])
@pytest.mark.parametrize("family", FULL_FAMILIES)
def test_evict_on_full_inside_the_stream(nf, O, lab, family, small, layout, batch, ingest_variant):
    """The whole eviction sequence, every eviction bit for bit: the cuts fall inside scripts, a flow's next record starts a NEW
    flow (another first record, stored whole), and the oracle decides. The optimistic fold, its rollback and the search for the
    split (one call) and the batched loop."""
    c = lab(family)
    max_entries = 50 if small else c.fam.n_scripts // 3
    try:
        want = check_against_oracle(nf, O, c.recs(layout), max_entries, batch, ingest_variant=ingest_variant)
    except AssertionError as e:
        raise AssertionError("%s, evict on full at %d, %s, batch %d, variant %d: %s" % (family, max_entries, layout, batch, ingest_variant, e)) from None
    fulls = [len(b) for r, b in want if r == "full"]
    print("%s, max_entries %d, %s: %d evictions on full" % (family, max_entries, layout, len(fulls)))
    assert len(fulls) >= 2 and all(k == max_entries for k in fulls)


# ---------------------------------------------------------------- 6: nfagg_account
PAR_FAMILIES = ("times", "lastnz", "macs")                   # calls large enough for csrc/nfagg_api_account.hip (account_par_min_records)
ACCOUNT_SIZES = [(f, third) for f in bc.FAMILIES for third in (False, True) if not (third and f == "hot")]      # eight flows: a third is two


@pytest.mark.parametrize("layout", ["shuffled", "round_major"])
@pytest.mark.parametrize("ingest_variant", [0, 30])
@pytest.mark.parametrize("family,third", ACCOUNT_SIZES, ids=["%s-%s" % (f, "third" if t else "never_full") for f, t in ACCOUNT_SIZES])
def test_account(nf, O, lab, family, third, ingest_variant, layout):
    """The record arm of Accounter.Account with its evictions on full, in one call: epochs found first (variant 0, where the call
    is large enough) and the kernel chain (30). max_entries = the scripts: the map is exactly full at the end and never evicts."""
    c = lab(family)
    max_entries = c.fam.n_scripts // 3 if third else c.fam.n_scripts
    recs = c.recs(layout)
    with nf.FlowTable(max_entries=max_entries, ingest_variant=ingest_variant) as tab:
        try:
            n_ev = check_account(nf, O, tab, recs, max_entries, [len(recs)])
        except AssertionError as e:
            raise AssertionError("%s, account, max_entries %d, %s, variant %d: %s" % (family, max_entries, layout, ingest_variant, e)) from None
        st = tab.stats()
        print("%s, account, max_entries %d, %s, variant %d: %d evictions; account_epochs_first %d, account_chain %d, account_declined %d"
              % (family, max_entries, layout, ingest_variant, n_ev, st.account_epochs_first, st.account_chain, st.account_declined))
        assert st.records_ingested == len(recs) and st.evictions[nf.REASON_FULL] == n_ev - 1
        assert (n_ev > 2) == third
        if ingest_variant == 30:
            assert st.account_epochs_first == 0 and st.account_chain > 0
        elif third and family in PAR_FAMILIES:
            assert st.account_epochs_first > 0, "the call was meant to have its epochs found first"


# ---------------------------------------------------------------- 7: ranks
@pytest.mark.parametrize("family", bc.FAMILIES)
def test_four_ranks_fold_the_rounds_in_turn(nf, lab, family):
    """Round j goes to rank j % 4 with its arrival position as sequence number: consecutive records of every flow lie on different
    ranks. Epoch 1: the ranks fold in ascending order. Epoch 2: in descending order — rank 0, which holds every flow's first
    record, folds last. Then the tick: k_export_*, k_merge_raw / k_merge_identity at the owners, the owned eviction."""
    c = lab(family)
    rounds = c.rounds()
    R = Ranks(nf, 4, max_entries=1 << 16)
    try:
        for order in ([0, 1, 2, 3], [3, 2, 1, 0]):
            for rank in order:
                for j in range(rank, len(rounds), 4):
                    R.fold(rank, rounds[j], int(c.bounds[j]))
            got, counts = R.tick()
            print("%s, four ranks %s: partials sent %s" % (family, order, [sum(x) for x in counts]))
            assert sum(map(sum, counts)) > 0
            c.check(got, "four ranks, folding in rank order %s" % order)
    finally:
        R.close()


@pytest.mark.parametrize("family", bc.FAMILIES)
def test_three_ranks_with_contiguous_slices(nf, lab, family):
    """Rank r folds arrival positions [r n, (r + 1) n) of the shuffled layout; two epochs."""
    c = lab(family)
    recs = c.recs("shuffled")
    per = len(recs) // 3
    want = c.oracle(recs[:3 * per])
    R = Ranks(nf, 3, max_entries=1 << 16)
    try:
        for epoch in range(2):
            for r in range(3):
                R.fold(r, recs[r * per:(r + 1) * per], r * per)
            got, counts = R.tick()
            assert sum(map(sum, counts)) > 0
            c.check(got, "three ranks with contiguous slices, epoch %d" % epoch, want)
    finally:
        R.close()


@pytest.mark.parametrize("family", bc.FAMILIES)
def test_four_ranks_restart_their_window_together(nf, lab, family):
    """The first half of the rounds, then the job's position leaps past every rank's window: the fold is refused, every rank
    exports ALL its flows grouped by owner, the owners restart at the common position (nfagg_window_restart_device: k_merge_sub*
    and the ranking of the merged slots), the second half is folded above it, and the tick ends the epoch."""
    import torch
    c = lab(family)
    rounds, n = c.rounds(), 4
    half = len(rounds) // 2
    leap = WINDOW - 1                           # no call fits behind it, however short (a round of `wave` has 64 records)
    R = Ranks(nf, n, max_entries=1 << 16)
    try:
        for j in range(half):
            R.fold(j % n, rounds[j], int(c.bounds[j]))
        with pytest.raises(nf.NfaggError) as ei:
            R.fold(half % n, rounds[half], leap)
        assert ei.value.code == -6 and "nfagg_window_restart_device" in str(ei.value)
        counts = []
        for r in range(n):
            rc, cnt, total = R.tabs[r].partials_export_device(n, 0xFFFFFFFF, R.exp[r].data_ptr(), R.exp[r].numel() // 24)
            assert rc == nf.OK
            counts.append(cnt)
        for owner in range(n):
            segs = [R.exp[src][sum(counts[src][:owner]) * 24:(sum(counts[src][:owner]) + counts[src][owner]) * 24] for src in range(n)]
            mine = torch.cat(segs)
            R.keep.append(mine)
            torch.cuda.synchronize()
            R.tabs[owner].window_restart_device(n, owner, mine.data_ptr(), mine.numel() // 24, leap)
        assert sum(len(t) for t in R.tabs) == int((c.fam.length > 0).sum())         # one slot per flow, at its owner
        for j in range(half, len(rounds)):
            R.fold(j % n, rounds[j], leap + int(c.bounds[j]))
        got, _ = R.tick()
        c.check(got, "four ranks restarting their window after round %d" % half)
    finally:
        R.close()


# ---------------------------------------------------------------- 8: a one-process group
@pytest.mark.parametrize("n_members", [2, 3])
@pytest.mark.parametrize("family", bc.FAMILIES)
def test_local_fold_group(nf, lab, family, n_members):
    """FlowGroup([0] * n, local_fold=True): round j is folded on member j % n, so consecutive records of every flow lie on
    different members; the eviction brings the members' slots to their owners and merges them."""
    import torch
    c = lab(family)
    keep = []
    with nf.FlowGroup([0] * n_members, max_entries=1 << 16, local_fold=True) as grp:
        for j, r in enumerate(c.rounds()):
            d = torch.from_numpy(np.ascontiguousarray(r).view(np.uint8).reshape(-1).copy()).cuda()
            torch.cuda.synchronize()
            keep.append(d)
            assert grp.ingest_device(j % n_members, d.data_ptr(), len(r)) == (nf.OK, len(r))
        assert all(m.stats().records_ingested > 0 for m in grp.members)
        got = nf.sort_by_key(grp.evict(nf.REASON_TIMEOUT))
    c.check(got, "local-fold group of %d" % n_members)
