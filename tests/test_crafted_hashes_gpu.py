"""Fold parity on CRAFTED key hashes. Every other fold test feeds keys whose 64-bit hashes are effectively random: no test gives a
kernel two flows with one hash, a probe chain of hundreds of slots, or a hash on a field boundary. tests/keycraft.py builds a key
for any hash; here whole families of such keys are planted into a seeded stream — half of a family's flows on the stream's hottest
ranks (they live in the LDS caches), half on cold ones of a few records (spilled, bypassed) — and the stream goes through the
smallest shape that reaches each kernel. The expected result is always the oracle's Accounter, bit for bit.

    same64          groups of 2, 3 and 40 flows per hash (eight groups): every full-key compare behind a hash match
    bit0            50 pairs h, h ^ 1: the LDS caches store h | 1 — one cache entry, two home slots
    one_home_ones   300 flows with equal low 21 bits, all ones: a probe chain from the table's last slot round to slot 0, one partition
    one_home_m5     ... low bits mask - 5: the chain starts five slots before the end
    same_fp         bits 18..63 equal, 2 x window consecutive home slots across a pass-2 partition border: equal fingerprints
                    (equal `locked` / `ready` tags) in adjacent slots, one LDS probe window overfull
    cache_wrap      LDS home entries kEntries - 2 and kEntries - 1, 2 x window flows each: LDS probing wraps to entry 0
    edge            hashes 0, 1, 2, 3, 2^63, 2^64 - 2, 2^64 - 1, some of them shared: the free marker 0, the busy marker 2, all-ones fields
    one_bit         no crafting: a key, its 312 single-bit neighbours (four pairs of which share their hash, see
                    tests/test_keycraft_cpu.py), byte 39 flipped eight ways; random full-width keys for every other flow
    shard_edge      upper hash halves on both sides of every boundary of the shard formula (a test of its own)

The windows and cache sizes come from csrc/ (keycraft.fold_constants), the table's mask from stats().table_slots."""
import numpy as np
import pytest

import keycraft as kc
from conftest import assert_records_equal, dedup_stream
from test_dedup_gpu import check_dedup
from test_parity_gpu import check_against_oracle
from test_partials_gpu import ranks_with_contiguous_slices

pytestmark = pytest.mark.gpu

MIN_ENTRIES = 1 << 15                       # the smallest table: 2^16 slots


class Lab:
    """Streams and oracle results, built once per (family, kind of stream, table mask)."""

    def __init__(self, nf, O):
        self.nf, self.O = nf, O
        self.consts = kc.fold_constants()
        self.th = O.zipf_thresholds(kc.N_FLOWS, 1.1)
        self._base, self._fam, self._mask = {}, {}, {}

    def base(self, kind):
        """kind: "acc" (stream variant 1) or "dd1" / "dd2" (conftest.dedup_stream styles 1 and 2)."""
        if kind not in self._base:
            if kind == "acc":
                b = self.O.gen_stream(kc.N_RECORDS, seed=300, n_keys=kc.N_FLOWS, thresholds=self.th, variant=1)
            else:
                b = dedup_stream(self.O, kc.N_RECORDS, seed=300 + int(kind[2]), n_keys=kc.N_FLOWS, thresholds=self.th, style=int(kind[2]))
            self._base[kind] = b
        return self._base[kind]

    def mask(self, **table_kw):
        key = tuple(sorted(table_kw.items()))
        if key not in self._mask:
            with self.nf.FlowTable(max_entries=MIN_ENTRIES, **table_kw) as tab:
                self._mask[key] = int(tab.stats().table_slots) - 1
        return self._mask[key]

    def family(self, name, kind, mask=None):
        """(records, the oracle's single eviction, planted keys)."""
        mask = self.mask() if mask is None else mask
        key = (name, kind, mask)
        if key not in self._fam:
            if name.startswith("shard_edge"):
                recs, keys, _ = kc.apply_shard_edge(self.base(kind), int(name[10:]))
            else:
                recs, keys, _ = kc.apply_family(self.base(kind), name, mask, self.consts)
            want = self.O.run_accounter(recs, 1 << 20, 0 if kind == "acc" else 1)
            assert len(want) == 1 and len(want[0][1]) == kc.distinct_flows(recs)
            self._fam[key] = (recs, want[0][1], keys)
        return self._fam[key]


@pytest.fixture(scope="module")
def lab(nf, O):
    return Lab(nf, O)


def fold_and_evict(nf, recs, batch=None, **table_kw):
    """One table, the stream in one call or in batches, one eviction. Returns (evicted records sorted by key, stats before the eviction)."""
    view = recs.view(nf.FLOW_RECORD)
    batch = batch or len(view)
    with nf.FlowTable(**table_kw) as tab:
        for lo in range(0, len(view), batch):
            assert tab.ingest(view[lo:lo + batch]) == (nf.OK, len(view[lo:lo + batch]))
        n_live = len(tab)
        st = tab.stats()
        got = nf.sort_by_key(tab.evict(nf.REASON_CLOSING))
        assert len(got) == n_live
        return got, st


def check_one_home(name, st, what):
    """K flows share ONE home slot: whichever of them was placed furthest has walked past the K - 1 others in one lookup."""
    if name.startswith("one_home"):
        print("%s: max_probe %d (precondition: >= %d)" % (what, st.max_probe, kc.ONE_HOME_K - 1))
        assert st.max_probe >= kc.ONE_HOME_K - 1, "the flows were meant to share one home slot"


def tiles_with_colliders(recs, keys, at_least):
    """1024-record tiles (what a pass-1 workgroup folds at a time) that hold records of `at_least` flows of ONE hash among `keys`."""
    h = kc.key_hash(kc.as_words(keys))
    group = {bytes(k[:39]): int(x) for k, x in zip(keys, h) if (h == x).sum() >= at_least}
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), 144)[:, :39]
    n = 0
    for lo in range(0, len(raw), 1024):
        seen = {}
        for k in raw[lo:lo + 1024]:
            g = group.get(bytes(k))
            if g is not None:
                seen.setdefault(g, set()).add(bytes(k))
        n += any(len(v) >= at_least for v in seen.values())
    return n


# ---------------------------------------------------------------- accounter mode, the smallest table
@pytest.mark.parametrize("ingest_variant,batch", [(1, None), (3, None), (7, None), (10, None), (11, None), (17, None), (7, 257), (10, 257)])
@pytest.mark.parametrize("family", kc.FAMILIES)
def test_accounter_routes(nf, lab, family, ingest_variant, batch):
    """The direct kernel (1), the single-pass cached kernels (3: 512 entries, 7: 1024), the two-pass fold (10; 11 without its
    admission filter; 17 with the pass 1 that publishes its entries) on a table of 2^16 slots.

    Precondition of same64 on variant 10 in one call — the record-by-record merge of pass 2 (pass2_round's non-RETRY branch,
    upsert_partial in a kernel whose flushes are plain read-modify-write) is reached: a pass-1 workgroup keeps ONE cache entry per
    hash, the entry holds one flow's key, and every record of another flow with that hash fails cache_fold's full-key compare and
    is spilled. The stream has tiles of 1024 records (a workgroup folds whole tiles) with four or more flows of one 40-group, so
    at least three flows of one hash meet in one pass-2 queue. There the first to claim the entry holds it, the records of the
    others miss and go to the retry list; all have one hash, hence one sub-partition and one retry round with a fresh cache, where
    again one flow holds the entry and the rest miss — with no further round to go to, they are merged record by record."""
    recs, want, keys = lab.family(family, "acc")
    got, st = fold_and_evict(nf, recs, batch, max_entries=MIN_ENTRIES, ingest_variant=ingest_variant)
    what = "%s variant %d batch %s" % (family, ingest_variant, batch)
    check_one_home(family, st, what)
    if family == "same64" and ingest_variant == 10 and batch is None:
        n_tiles = tiles_with_colliders(recs, keys, 4)
        print("%s: %d tiles hold 4+ flows of one hash; records_bypassed %d (precondition: > 0)" % (what, n_tiles, st.records_bypassed))
        assert n_tiles > 0 and st.records_bypassed > 0
    assert_records_equal(got, want, what)


# ---------------------------------------------------------------- accounter mode, a table with deferred claims
@pytest.mark.parametrize("ingest_variant", [10, 17])
@pytest.mark.parametrize("family", ["same64", "same_fp", "one_home_ones", "one_home_m5"])
def test_two_pass_fold_with_deferred_claims(nf, lab, family, ingest_variant):
    """2^21 slots: pass 2 claims per workgroup (find_or_claim<DEFER>: a slot being claimed is another flow's whatever its
    fingerprint — move on). The partition is bits 10..20 of the hash then, the sub-partition bits 7..9; one_home and same_fp are
    built from this table's mask."""
    mask = lab.mask(table_log2_slots=21)
    assert mask == (1 << 21) - 1
    recs, want, _ = lab.family(family, "acc", mask)
    got, st = fold_and_evict(nf, recs, None, max_entries=MIN_ENTRIES, table_log2_slots=21, ingest_variant=ingest_variant)
    what = "%s variant %d, 2^21 slots" % (family, ingest_variant)
    check_one_home(family, st, what)
    assert_records_equal(got, want, what)


# ---------------------------------------------------------------- kernel-dedup mode
@pytest.mark.parametrize("style", [1, 2])
@pytest.mark.parametrize("ingest_variant", [1, 10, 12, 16])
@pytest.mark.parametrize("family", ["same64", "bit0", "same_fp", "one_home_ones", "one_home_m5"])
def test_dedup_routes(nf, lab, family, ingest_variant, style):
    """The direct dedup kernels (1) and the cached passes (10; 12 without retry rounds; 16 sorting first). Their LDS caches are
    keyed by (flow hash, interface): flows with one hash on one interface share a cache hash, and same_subflow's compare of the
    five key words is all that keeps them apart."""
    recs, want, _ = lab.family(family, "dd%d" % style)
    got, st = fold_and_evict(nf, recs, None, max_entries=MIN_ENTRIES, mode=nf.MODE_KERNEL_DEDUP, ingest_variant=ingest_variant)
    what = "dedup %s variant %d style %d" % (family, ingest_variant, style)
    check_one_home(family, st, what)
    assert_records_equal(got, want, what)


# ---------------------------------------------------------------- evict on full inside the batch
@pytest.mark.parametrize("mode", ["accounter", "dedup"])
@pytest.mark.parametrize("ingest_variant", [0, 10])
@pytest.mark.parametrize("max_entries,batch", [(50, 4096), (999, 1 << 30)])
def test_evict_on_full_with_colliding_flows(nf, O, lab, max_entries, batch, ingest_variant, mode):
    """The optimistic fold, its rollback and the search for the split with flows that share their hash: every eviction holds
    exactly max_entries flows, colliders counted one by one."""
    recs, _, _ = lab.family("same64", "acc" if mode == "accounter" else "dd2")
    check = check_against_oracle if mode == "accounter" else check_dedup
    want = check(nf, O, recs, max_entries, batch, ingest_variant=ingest_variant)
    assert sum(1 for r, _ in want if r == "full") >= 2 and all(len(b) == max_entries for r, b in want if r == "full")


# ---------------------------------------------------------------- sketches
@pytest.mark.parametrize("mode", ["accounter", "dedup"])
def test_sketches_with_colliding_flows(nf, O, lab, mode):
    """The fused sketch updates take their addresses from the cache entry (or the record) they flush: a collider that was turned
    away from an entry must still feed ITS addresses. Count-Min d = 4, w = 2^12, HyperLogLog p = 10, all four against the oracle."""
    recs, want, _ = lab.family("same64", "acc" if mode == "accounter" else "dd2")
    kw = dict(mode=nf.MODE_KERNEL_DEDUP) if mode == "dedup" else {}
    with nf.FlowTable(max_entries=MIN_ENTRIES, ingest_variant=10, sketches=nf.SKETCH_CM | nf.SKETCH_HLL, cm_depth=4, cm_log2_width=12, hll_p=10, **kw) as tab:
        assert tab.ingest(recs.view(nf.FLOW_RECORD)) == (nf.OK, len(recs))
        snap = [tab.sketch_snapshot(w) for w in (nf.CM_SRC, nf.CM_DST, nf.HLL_SRC, nf.HLL_DST)]
        got = nf.sort_by_key(tab.evict(nf.REASON_CLOSING))
    for g, w, name in zip(snap, O.sketches(recs, 4, 12, 10), ("cm src", "cm dst", "hll src", "hll dst")):
        assert np.array_equal(g, w), name
    assert_records_equal(got, want, "sketches, " + mode)


# ---------------------------------------------------------------- shards
@pytest.mark.parametrize("ingest_variant", [1, 7, 10])
@pytest.mark.parametrize("n_shards", [3, 8])
def test_sharded_tables_on_the_shard_boundaries(nf, lab, n_shards, ingest_variant):
    """One table per shard over a stream whose planted hashes sit on both sides of every boundary of shard_of_hash: each shard
    evicts exactly the flows the formula (in Python integers) gives it, the union is the oracle's, the skipped records add up."""
    recs, want, _ = lab.family("shard_edge%d" % n_shards, "acc")
    owner = kc.shard_formula(want, n_shards)
    parts, skipped = [], 0
    for s in range(n_shards):
        with nf.FlowTable(max_entries=MIN_ENTRIES, n_shards=n_shards, shard_id=s, ingest_variant=ingest_variant) as tab:
            assert tab.ingest(recs.view(nf.FLOW_RECORD)) == (nf.OK, len(recs))
            ev = nf.sort_by_key(tab.evict())
            skipped += tab.stats().records_skipped
        assert (kc.shard_formula(ev, n_shards) == s).all()
        assert_records_equal(ev, want[owner == s], "shard %d of %d" % (s, n_shards))
        parts.append(ev)
    assert skipped == (n_shards - 1) * len(recs)
    assert_records_equal(nf.sort_by_key(np.concatenate(parts)), want)


# ---------------------------------------------------------------- local fold: one process (group), several processes (partials)
@pytest.mark.parametrize("mode", ["accounter", "dedup"])
@pytest.mark.parametrize("family", ["same64", "shard_edge4"])
def test_local_fold_group(nf, lab, family, mode):
    """FlowGroup([0] * 4, local_fold=True): the chunks go round the members, a flow lives on several of them (sub-flow tables in
    kernel-dedup mode) and the eviction merges the members' slots into their owners — by key, whatever the hashes."""
    recs, want, _ = lab.family(family, "acc" if mode == "accounter" else "dd2")
    kw = dict(mode=nf.MODE_KERNEL_DEDUP) if mode == "dedup" else {}
    with nf.FlowGroup([0] * 4, max_entries=1 << 16, local_fold=True, staging_records=7_000, **kw) as grp:
        assert grp.ingest(recs.view(nf.FLOW_RECORD)) == (nf.OK, len(recs))
        assert all(m.stats().records_ingested > 0 for m in grp.members)
        got = nf.sort_by_key(grp.evict(nf.REASON_TIMEOUT))
    assert_records_equal(got, want, "local-fold group, %s, %s" % (family, mode))


@pytest.mark.parametrize("family", ["same64", "same_fp", "shard_edge4"])
def test_partials_between_four_ranks(nf, O, lab, family):
    """Four handles as the ranks of a local-fold job: export, merge, evict_owned (tests/test_partials_gpu.py's driver). The
    ranks' tables have 2^20 slots: same_fp is built from their mask."""
    recs, _, _ = lab.family(family, "acc", (1 << 20) - 1)
    ranks_with_contiguous_slices(nf, O, recs, 4)
