// nfagg_api.hip — the flow table behind the C ABI of libnfagg (include/nfagg.h): handle, pinned
// staging ring, batch control flow of Accounter.Account
// (pkg/flow/account.go:58-100) around the kernels. No CPU fallback: without a
// gfx950 device nfagg_create fails. The handle owns its resources through the owner types of nfagg_handle.h: nothing is
// freed by hand here, nfagg_destroy deletes the handle. The rest of the ABI's host side: nfagg_api_account.hip (nfagg_account*:
// the record arm with its evictions on full) and nfagg_api_group.hip (the multi-GPU group), which drive the handle through the
// functions declared in nfagg_api_core.h; nfagg_api_export.hip (the encoders), nfagg_api_tables.hip (the caller tables),
// nfagg_api_aux.hip (rollups, map merge, sketches).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"
#include "nfagg_handle.h"
#include "nfagg_api_core.h"
#include "nfagg_hostpool.h"

using namespace nfagg;

static_assert(sizeof(nfagg_flow_id) == 40, "flow_id");
static_assert(sizeof(nfagg_flow_metrics) == 104, "flow_metrics");
static_assert(sizeof(nfagg_flow_record) == 144, "flow_record");
static_assert(sizeof(nfagg_additional_metrics) == 32, "additional");
static_assert(sizeof(nfagg_dns_metrics) == 64, "dns");
static_assert(sizeof(nfagg_pkt_drop_metrics) == 32, "drops");
static_assert(sizeof(nfagg_network_events_metrics) == 72, "netev");
static_assert(sizeof(nfagg_xlat_metrics) == 56, "xlat");
static_assert(sizeof(nfagg_quic_metrics) == 24, "quic");

namespace {

thread_local std::string g_create_error;

}  // namespace

// Declared in nfagg_handle.h: the other host files of the ABI report errors through this.
namespace nfagg {

int fail(nfagg_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) { std::lock_guard<std::mutex> lk(h->err_mu); h->err = buf; } else g_create_error = buf;
    return code;
}

// --- profiling: HIP events on the handle's stream around the dominant kernels
void prof_begin(nfagg_handle* h, EventPair& ep, int kind) {
    if (h->ev_free.empty()) {
        for (hipEvent_t* e : {&ep.a, &ep.b}) { h->ev_pool.emplace_back(); h->ev_pool.back().create(hipEventDefault); *e = h->ev_pool.back(); }
    } else { ep = h->ev_free.back(); h->ev_free.pop_back(); }
    ep.kind = kind;
    hipEventRecord(ep.a, h->stream);
}
void prof_end(nfagg_handle* h, EventPair& ep) {
    hipEventRecord(ep.b, h->stream);
    h->ev_pending.push_back(ep);
}
void prof_resolve(nfagg_handle* h) {
    for (auto& ep : h->ev_pending) {
        hipEventSynchronize(ep.b);
        float ms = 0.f;
        hipEventElapsedTime(&ms, ep.a, ep.b);
        if (ep.kind == 0) { h->stats.ingest_kernel_ms += ms; h->stats.ingest_launches++; }
        else if (ep.kind == 1) { h->stats.evict_kernel_ms += ms; h->stats.evict_launches++; }
        else { h->stats.sketch_kernel_ms += ms; h->stats.sketch_launches++; }
        h->ev_free.push_back(ep);
    }
    h->ev_pending.clear();
}

int launch_ingest_profiled(nfagg_handle* h, const void* d, uint64_t n, uint64_t seq_base) {
    EventPair ep{};
    h->counters_exact = false; h->mirror_fresh = false;      // callers that know the outcome set counters_exact again
    const bool prof = h->cfg.profile != 0;
    if (!ingest_needs_spill((int)h->cfg.mode, (int)h->cfg.ingest_variant, n)) h->epoch_unclustered = true;
    if (ingest_needs_spill((int)h->cfg.mode, (int)h->cfg.ingest_variant, n)) {
        // room for twice the even share of a batch in which every record spills; beyond that the kernel merges directly
        uint64_t qcap = (2 * n / kSpillParts + 1024 + 3) & ~3ull;
        // overflow list: every item (record; kernel-dedup mode: or exported cache entry) may overflow, ONE slot each
        // (overflow_push_one), plus one padded group per partition per workgroup
        const uint64_t ovf_cap = ((n + 3) & ~3ull) + kDedupXpEntries + 256ull * kSpillParts * 4;
        if (qcap > h->tv.spill.qcap || ovf_cap > h->tv.spill.ovf_cap) {
            if (qcap < h->tv.spill.qcap) qcap = h->tv.spill.qcap;
            const size_t qbytes = (size_t)kSpillParts * qcap * sizeof(uint32_t);
            int rc = h->spill_queues.ensure(h, qbytes + ovf_cap * sizeof(uint32_t));
            if (rc != NFAGG_OK) return rc;
            h->tv.spill.queue = h->spill_queues.as<uint32_t>();
            h->tv.spill.qcap = (uint32_t)qcap;
            h->tv.spill.ovf = (uint32_t*)(h->spill_queues.as<char>() + qbytes);
            h->tv.spill.ovf_cap = (uint32_t)((h->spill_queues.cap - qbytes) / sizeof(uint32_t) > 0xfffffff0ull ? 0xfffffff0ull
                                             : ((h->spill_queues.cap - qbytes) / sizeof(uint32_t)) & ~3ull);
        }
        if (h->cfg.mode == NFAGG_MODE_KERNEL_DEDUP) {
            // the partition pass sorts its items by sub-partition first when a partition's flows will not fit one cache (1024
            // sub-flow entries x 2048 partitions): the last epoch's flow count is the guess, the table's size before there is one
            const uint64_t guess = h->last_epoch_flows ? h->last_epoch_flows * (h->tv.subflow ? 1 : 2) : (h->cfg.max_entries > (1ull << 22) ? ~0ull : 0ull);
            h->tv.spill.sort_first = h->cfg.ingest_variant == kVariantDedupSortFirst ? 2u : (guess > 2500000ull ? 1u : 0u);    // 2: whatever the partition's size (tests)      // ~1200 sub-flows per partition: one cache (and its retry round) still holds them
        }
        if (h->cfg.mode == NFAGG_MODE_KERNEL_DEDUP && !h->tv.spill.xp) {     // exported cache entries of the streaming pass (38 MB)
            int rc = h->spill_xp.ensure(h, (size_t)kDedupXpBytes);
            if (rc != NFAGG_OK) return rc;
            h->tv.spill.xp = h->spill_xp.as<uint4>();
        }
    }
    if (prof) { if (h->ev_pending.size() >= 8192) prof_resolve(h); prof_begin(h, ep, 0); }
    const uint64_t rel = seq_base - h->seq_origin;              // what the slots' 32-bit tags carry (callers keep rel + n inside the window)
    hipError_t e = launch_ingest(h->tv, h->sk, d, n, rel, (int)h->cfg.mode, (int)h->cfg.ingest_variant, h->stream);
    // identity dwords of the flows this batch created, from the batch (the caller owns it until the call returns)
    if (e == hipSuccess) e = launch_finalize(h->tv, d, n, rel, h->stream);
    if (prof) prof_end(h, ep);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "ingest launch failed: %s", hipGetErrorString(e));
    if (h->sk.flags && !ingest_fuses_sketches((int)h->cfg.mode, (int)h->cfg.ingest_variant, n, h->sk.flags)) {
        if (prof) prof_begin(h, ep, 2);
        e = launch_sketch_update(h->sk, h->tv, d, n, h->stream);
        if (prof) prof_end(h, ep);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "sketch launch failed: %s", hipGetErrorString(e));
    }
    return NFAGG_OK;
}

// Bring the device counters to the host (synchronises the stream). In two halves for callers that wait for something else on the
// same stream anyway: enqueue the copy, wait once, take the counters in.
int refresh_counters_enqueue(nfagg_handle* h) {
    HIP_TRY(h, hipMemcpyAsync(h->h_ctr, h->tv.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, h->stream));
    return NFAGG_OK;
}
int refresh_counters_taken(nfagg_handle* h) {
    if (h->h_ctr->error)
        return fail(h, NFAGG_EDEVICE, "flow table kernel bailed out (code %u: 1 = probe overflow / table too small, 2 = claim spin limit, 5 = spill overflow list full, 6 = claimed slot without a record, 7 = partial of another shard merged)", h->h_ctr->error);
    h->live_ub = h->h_ctr->n_live;
    if (!h->must_evict) h->live = h->h_ctr->n_live;
    h->counters_exact = true; h->mirror_fresh = true;
    h->stats.records_skipped = h->h_ctr->n_skipped;
    h->stats.records_bypassed = h->h_ctr->n_bypassed;
    if (h->h_ctr->max_probe > h->stats.max_probe) h->stats.max_probe = h->h_ctr->max_probe;
    return NFAGG_OK;
}
int refresh_counters(nfagg_handle* h) {
    int rc = refresh_counters_enqueue(h);
    if (rc != NFAGG_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return refresh_counters_taken(h);
}

// ---- optimistic fold -------------------------------------------------------------------------------------------
// A batch that MIGHT reach `len(entries) >= maxEntries` at a new key (account.go:85) — live + batch > max_entries — is
// folded whole, by the same kernels as any other batch, and checked afterwards: the sequential Accounter finds the table
// full iff the number of distinct keys (live + new ones of the batch) exceeds max_entries, so `n_live <= max_entries`
// after the fold proves that no record of the batch triggered the eviction, and the fold stands as it is. Otherwise
// the fold is rolled back — the slots claimed by the batch are zeroed, the slots that were live before it are restored
// from a raw copy taken before the fold, the sketches from theirs — and the exact split point is read off the table: every
// slot carries its flow's first sequence number (the tag of id0), so the record whose new key finds the table full is the
// (room+1)-th smallest first sequence number among the slots the batch claimed. The prefix before it is folded again
// (now exactly `room` new keys: it fits), the caller gets NFAGG_FULL + consumed as the reference's eviction demands.
// Claims are bounded by TableView.claim_limit whatever the batch holds: a batch with more new keys than the table has
// room for is `aborted` by the kernels (some claims refused), rolled back the same way and retried with a quarter of it.
constexpr size_t kCarefulCountsBytes = 256;    // h_careful: block counts of a small chunk (16 x 4 bytes), then its flags
constexpr uint64_t kCarefulMaxBatch = 16384;   // below this the claim + flag path decides (two small launches, one host round trip)

// ---- the sequence window (nfagg_rebase.hip) --------------------------------------------------------------------
constexpr uint64_t kSeqWindow = 0xFFFFFFF0ull;     // relative sequence numbers stay below this
constexpr uint64_t kMaxFoldChunk = 1ull << 31;     // records per pass of the ingest loop: always fits a fresh window

// Make room for `n` (<= kMaxFoldChunk) more sequence numbers. A table that holds the only copy of its flows rebases its tags in
// place; a handle whose numbering is shared with other tables (local fold across GPUs) cannot: *blocked tells the caller.
int ensure_seq_window(nfagg_handle* h, uint64_t n, bool* blocked) {
    if (blocked) *blocked = false;
    if (h->epoch_seq - h->seq_origin + n < kSeqWindow) return NFAGG_OK;
    // (a sub-flow table cannot either: the order BETWEEN the slots of one flow matters until the join, ranks inside a slot lose it)
    if (h->ext_sequenced || h->tv.subflow) { if (blocked) *blocked = true; return NFAGG_OK; }
    const hipError_t e = launch_rebase(h->tv, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "rebase launch failed: %s", hipGetErrorString(e));
    h->seq_origin = h->epoch_seq - rebase_keep();
    h->stats.sequence_rebases++;
    h->mirror_fresh = h->mirror_fresh;                          // counters untouched: the live list and n_live stay as they are
    return NFAGG_OK;
}

int snapshot_sketches(nfagg_handle* h, bool restore) {
    if (!h->sk.flags) return NFAGG_OK;
    const size_t cmb = (h->sk.flags & NFAGG_SKETCH_CM) ? ((size_t)h->sk.cm_depth << h->sk.cm_log2w) * sizeof(uint64_t) : 0;
    const size_t hlb = (h->sk.flags & NFAGG_SKETCH_HLL) ? ((size_t)1 << h->sk.hll_p) : 0;      // one byte per register
    int rc = h->opt.sketches.ensure(h, 2 * (cmb + hlb));
    if (rc != NFAGG_OK) return rc;
    char* snap = h->opt.sketches.as<char>();
    for (int k = 0; k < 2; k++) {
        if (cmb) HIP_TRY(h, restore ? hipMemcpyAsync(h->sk.cm[k], snap + k * cmb, cmb, hipMemcpyDeviceToDevice, h->stream)
                                    : hipMemcpyAsync(snap + k * cmb, h->sk.cm[k], cmb, hipMemcpyDeviceToDevice, h->stream));
        if (hlb) HIP_TRY(h, restore ? hipMemcpyAsync(h->sk.hll[k], snap + 2 * cmb + k * hlb, hlb, hipMemcpyDeviceToDevice, h->stream)
                                    : hipMemcpyAsync(snap + 2 * cmb + k * hlb, h->sk.hll[k], hlb, hipMemcpyDeviceToDevice, h->stream));
    }
    return NFAGG_OK;
}

// The pieces of an optimistic fold (also driven member by member by the multi-GPU group, nfagg_api_group.hip):
//   opt_begin    raw copy of the live slots and of the sketches (h->live exact on entry: the caller refreshed the counters)
//   opt_fold     the fold itself, asynchronous, sequence numbers from h->epoch_seq
//   opt_result   waits; did the chunk cross max_entries / was it aborted; if it crossed: the index (relative to the
//                chunk) of the record whose new key found the table full — the (room+1)-th smallest first sequence
//                number among the slots the chunk claimed
//   opt_commit   the fold stands: account for it
//   opt_rollback table, sketches and counters as opt_begin found them
int opt_begin(nfagg_handle* h, OptState& st) {
    const uint64_t maxe = h->cfg.max_entries;
    st.old_live = h->live; st.seq0 = h->epoch_seq;
    st.room = maxe > st.old_live ? maxe - st.old_live : 0;
    st.before = *h->h_ctr;
    st.was_unclustered = h->epoch_unclustered;
    int rc;
    if (st.old_live) {
        if ((rc = h->opt.slots.ensure(h, snapshot_bytes(h->tv, st.old_live))) != NFAGG_OK) return rc;
        hipError_t e = launch_snapshot(h->tv, st.old_live, h->opt.slots.p, false, h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "snapshot launch failed: %s", hipGetErrorString(e));
    }
    return snapshot_sketches(h, false);
}

int opt_fold(nfagg_handle* h, const OptState& st, const void* d, uint64_t chunk) {
    return chunk ? launch_ingest_profiled(h, d, chunk, st.seq0) : NFAGG_OK;
}

int opt_result(nfagg_handle* h, OptState& st, uint64_t chunk, bool* crossed, bool* aborted, uint64_t* split) {
    int rc = refresh_counters(h);
    if (rc != NFAGG_OK) return rc;
    const uint64_t maxe = h->cfg.max_entries;
    st.n_after = h->h_ctr->n_live;
    *aborted = h->h_ctr->aborted != 0;
    *crossed = *aborted || st.n_after > maxe;
    *split = 0;
    h->stats.optimistic_folds++;
    if (!*crossed || *aborted) return NFAGG_OK;
    const uint64_t m = st.n_after - st.old_live;               // slots claimed by the chunk; m > room
    size_t temp_bytes = 0;
    hipError_t e = launch_sort_u32(nullptr, nullptr, m, nullptr, &temp_bytes, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "sort size query failed: %s", hipGetErrorString(e));
    if ((rc = h->opt.first_seqs.ensure(h, 2 * m * sizeof(uint32_t))) != NFAGG_OK) return rc;
    if ((rc = h->opt.sort_tmp.ensure(h, temp_bytes + 16)) != NFAGG_OK) return rc;
    uint32_t* seqs = h->opt.first_seqs.as<uint32_t>();
    e = launch_first_seqs(h->tv, st.old_live, st.n_after, seqs, h->stream);
    if (e == hipSuccess) e = launch_sort_u32(seqs, seqs + m, m, h->opt.sort_tmp.p, &temp_bytes, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "split search failed: %s", hipGetErrorString(e));
    uint32_t split_seq = 0;
    HIP_TRY(h, hipMemcpyAsync(&split_seq, seqs + m + st.room, sizeof split_seq, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const uint64_t rel0 = st.seq0 - h->seq_origin;              // the slots carry window-relative numbers
    if ((uint64_t)split_seq < rel0 || (uint64_t)split_seq - rel0 >= chunk)
        return fail(h, NFAGG_EDEVICE, "optimistic fold: split sequence %u outside the batch [%llu, %llu)", split_seq,
                    (unsigned long long)rel0, (unsigned long long)(rel0 + chunk));
    *split = (uint64_t)split_seq - rel0;
    return NFAGG_OK;
}

void opt_commit(nfagg_handle* h, const OptState& st, uint64_t chunk) {
    h->live = h->live_ub = h->h_ctr->n_live;
    h->counters_exact = true; h->mirror_fresh = true;          // opt_result read the counters after the fold
    h->epoch_seq = st.seq0 + chunk;
    h->stats.records_ingested += chunk;
}

int opt_rollback(nfagg_handle* h, const OptState& st) {
    h->stats.optimistic_rollbacks++;
    hipError_t e = launch_discard(h->tv, st.old_live, st.n_after, h->stream);
    if (e == hipSuccess && st.old_live) e = launch_snapshot(h->tv, st.old_live, h->opt.slots.p, true, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "rollback launch failed: %s", hipGetErrorString(e));
    int rc = snapshot_sketches(h, true);
    if (rc != NFAGG_OK) return rc;
    *h->h_ctr = st.before;                                     // n_live, n_finalized, the diagnostic counters: as before the chunk
    HIP_TRY(h, hipMemcpyAsync(h->tv.ctr, h->h_ctr, sizeof(DevCounters), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));               // h_ctr is reused by the next refresh
    h->epoch_unclustered = st.was_unclustered;
    h->live = h->live_ub = st.old_live;
    return NFAGG_OK;
}

// Fold d[0..chunk) optimistically (h->live exact on entry). On return: *folded = records folded for good (the epoch's
// sequence and record counters advanced by them), *full = the record after them found the table full (account.go:85),
// *retry = nothing folded, try a shorter chunk.
int fold_optimistic(nfagg_handle* h, const void* d, uint64_t chunk, uint64_t* folded, bool* full, bool* retry) {
    *folded = 0; *full = false; *retry = false;
    OptState st;
    int rc;
    if ((rc = opt_begin(h, st)) != NFAGG_OK) return rc;
    if ((rc = opt_fold(h, st, d, chunk)) != NFAGG_OK) return rc;
    bool crossed = false, aborted = false;
    uint64_t split = 0;
    if ((rc = opt_result(h, st, chunk, &crossed, &aborted, &split)) != NFAGG_OK) return rc;
    if (!crossed) { opt_commit(h, st, chunk); *folded = chunk; return NFAGG_OK; }   // no record of the chunk found the table full
    if ((rc = opt_rollback(h, st)) != NFAGG_OK) return rc;
    if (aborted) { *retry = true; return NFAGG_OK; }
    if (split > 0 && (rc = launch_ingest_profiled(h, d, split, st.seq0)) != NFAGG_OK) return rc;
    h->live = h->live_ub = h->cfg.max_entries;                 // exactly `room` new keys in the prefix: len(entries) == maxEntries
    h->epoch_seq = st.seq0 + split;
    h->stats.records_ingested += split;
    *folded = split; *full = true;
    return NFAGG_OK;
}

int subflow_join_discard(nfagg_handle* h);

// The record arm of Accounter.Account (account.go:81-96) for a device-resident batch.
int ingest_device_core(nfagg_handle* h, const void* d_records, size_t n, size_t* consumed_out) {
    size_t consumed = 0;
    const uint64_t maxe = h->cfg.max_entries;
    const char* base = static_cast<const char*>(d_records);
    int rc = NFAGG_OK;
    if (h->must_evict || h->exported) { if (consumed_out) *consumed_out = 0; return n ? NFAGG_FULL : NFAGG_OK; }
    if (n && (rc = subflow_join_discard(h)) != NFAGG_OK) { if (consumed_out) *consumed_out = 0; return rc; }
    while (consumed < n) {
        uint64_t rem = n - consumed;
        if (rem > kMaxFoldChunk) rem = kMaxFoldChunk;
        {   // the epoch has no maximum length (account.go:58-100): when the 32-bit window of the tags is used up it is moved
            bool blocked = false;
            if ((rc = ensure_seq_window(h, rem, &blocked)) != NFAGG_OK) break;
            if (blocked && h->tv.subflow) {
                // kernel-dedup mode of a local-fold rank: the window does not move (include/nfagg.h, nfagg_config.local_fold) —
                // the epoch ends here, as it does when the table is full: the caller evicts and resubmits the rest
                h->must_evict = true; h->split_seq = h->epoch_seq;
                rc = NFAGG_FULL;
                break;
            }
            if (blocked) {
                // numbering shared with other tables (nfagg_set_sequence): the window can only move when the flows have been
                // brought together at their owners (nfagg_window_restart_device; the in-process group does it by itself)
                rc = fail(h, NFAGG_ERANGE, "sequence window used up on an externally sequenced handle: restart the window (nfagg_window_restart_device) or evict");
                break;
            }
        }
        const void* d = base + consumed * kRecordBytes;
        if (h->live_ub + rem <= maxe) {
            // no record of this batch can find len(entries) >= maxEntries (account.go:85)
            if ((rc = launch_ingest_profiled(h, d, rem, h->epoch_seq)) != NFAGG_OK) break;
            h->live_ub += rem; h->epoch_seq += rem; consumed += rem;
            h->stats.records_ingested += rem;
            continue;
        }
        if (!h->counters_exact && (rc = refresh_counters(h)) != NFAGG_OK) break;
        const uint64_t room = maxe > h->live ? maxe - h->live : 0;
        if (room >= rem) { h->live_ub = h->live; continue; }          // fits after all: the fast path above takes it
        // epochs shorter than a claim + flag chunk (tiny CACHE_MAX_FLOWS, the reference's default of 5000 among them): that path
        // finds the split with two small launches and one round trip, an optimistic fold would be rolled back every time
        const bool tiny_epochs = h->epoch_len_hint != 0 && h->epoch_len_hint <= kCarefulMaxBatch;
        if (rem > kCarefulMaxBatch && !tiny_epochs) {
            if (!h->mirror_fresh && (rc = refresh_counters(h)) != NFAGG_OK) break;      // the rollback restores *h_ctr
            // ---- optimistic path (see fold_optimistic). How much to try: everything, unless this stream has been stopping on
            // full. Then an epoch is about epoch_len_hint records long: stay clearly inside it while far from its end (the chunk
            // fits, nothing is thrown away), and go for the split with a short chunk when close — a chunk that crosses
            // max_entries is folded, rolled back and its prefix folded again, so it should not be much longer than that prefix.
            uint64_t chunk = rem;
            if (h->epoch_len_hint) {
                const uint64_t E = h->epoch_len_hint;
                uint64_t want;
                if (E >= (1ull << 22)) {
                    want = 2 * E;                                  // long epochs: one fold at full two-pass speed, the split, the prefix again
                } else {                                           // (measured: 2.6 against 1.9 G records/s at 6.6 M-record epochs)
                    const uint64_t target = E - E / 8;
                    const uint64_t tail = E > h->epoch_seq ? E - h->epoch_seq : 0;
                    uint64_t shortc = 2 * tail;                    // go for the split: about twice what is left of the epoch
                    const uint64_t floor_ = 2 * E < (1ull << 17) ? 2 * E : (1ull << 17);
                    if (shortc < floor_) shortc = floor_;
                    want = h->epoch_seq + (1ull << 16) < target ? target - h->epoch_seq : shortc;   // (0.66 against 0.33 G records/s at 0.6 M)
                }
                if (want <= kCarefulMaxBatch) want = kCarefulMaxBatch + 1;
                if (chunk > want) chunk = want;
            }
            if (h->abort_cap && chunk > h->abort_cap) chunk = h->abort_cap;
            uint64_t folded = 0; bool full = false, retry = false;
            if ((rc = fold_optimistic(h, d, chunk, &folded, &full, &retry)) != NFAGG_OK) break;
            if (retry) {
                // more new keys than the table takes (claim_limit): a quarter of it next, but never less than what cannot
                // abort at all — a chunk of claim_limit - live records claims at most that many slots
                const uint64_t safe = h->tv.claim_limit > h->live_ub ? h->tv.claim_limit - h->live_ub : 0;
                if (chunk <= safe) { rc = fail(h, NFAGG_EDEVICE, "optimistic fold aborted although the chunk fits the table"); break; }
                h->abort_cap = chunk / 4 > safe ? chunk / 4 : safe;
                continue;
            }
            consumed += folded;                                   // epoch_seq and the record counter advanced inside
            if (full) {
                h->epoch_len_hint = h->epoch_seq > 1 ? h->epoch_seq : 1;      // this epoch took that many records
                h->must_evict = true; h->split_seq = h->epoch_seq;
                rc = NFAGG_FULL;
                break;
            }
            continue;
        }
        if (room >= 65536 || (room > 0 && room >= rem / 4)) {
            // the first `room` records cannot overflow either
            if ((rc = launch_ingest_profiled(h, d, room, h->epoch_seq)) != NFAGG_OK) break;
            h->live_ub += room; h->epoch_seq += room; consumed += room;
            h->stats.records_ingested += room;
            continue;
        }
        // ---- careful path (small batches): the split point may lie inside this chunk
        const uint64_t chunk = rem < h->careful_chunk ? rem : h->careful_chunk;
        const uint64_t seq0 = h->epoch_seq;
        h->epoch_unclustered = true;
        hipError_t e = launch_claim(h->tv, d, chunk, seq0 - h->seq_origin, h->d_slot_idx.as<uint32_t>(), h->stream);
        if (e == hipSuccess) e = launch_first_flags(h->tv, h->d_slot_idx.as<uint32_t>(), chunk, seq0 - h->seq_origin, h->d_flags.as<uint8_t>(), h->d_block_counts.as<uint32_t>(), h->stream);
        if (e != hipSuccess) { rc = fail(h, NFAGG_EDEVICE, "claim launch failed: %s", hipGetErrorString(e)); break; }
        const uint64_t nblk = (chunk + kFlagBlock - 1) / kFlagBlock;
        h->h_block_counts.resize(nblk);
        h->mirror_fresh = false;
        // small chunks (every chunk of a stream with tiny epochs): counts and flags come back together, one round trip
        const bool one_trip = chunk <= kCarefulMaxBatch;
        uint32_t* counts_dst = one_trip ? reinterpret_cast<uint32_t*>(h->h_careful) : h->h_block_counts.data();
        e = hipMemcpyAsync(counts_dst, h->d_block_counts.p, nblk * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && one_trip) e = hipMemcpyAsync(h->h_careful + kCarefulCountsBytes, h->d_flags.p, chunk, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) { rc = fail(h, NFAGG_EDEVICE, "claim sync failed: %s", hipGetErrorString(e)); break; }
        if (one_trip) memcpy(h->h_block_counts.data(), counts_dst, nblk * sizeof(uint32_t));
        uint64_t total_new = 0;
        for (uint64_t b = 0; b < nblk; b++) total_new += h->h_block_counts[b];
        if (h->live + total_new <= maxe) {
            if ((rc = launch_ingest_profiled(h, d, chunk, seq0)) != NFAGG_OK) break;
            h->live += total_new; h->live_ub = h->live; h->epoch_seq += chunk; consumed += chunk;
            h->stats.records_ingested += chunk;
            h->counters_exact = true;                              // n_live = live: every claimed slot is a flow of the epoch
            continue;
        }
        // The (room+1)-th new key of the chunk arrives with the table full:
        // everything before it is folded, then the caller must evict ("full").
        uint64_t want = room + 1, blk = 0, before = 0;
        while (before + h->h_block_counts[blk] < want) { before += h->h_block_counts[blk]; blk++; }
        uint8_t fl_buf[kFlagBlock];
        const uint64_t off = blk * kFlagBlock;
        const uint64_t cnt = (chunk - off) < (uint64_t)kFlagBlock ? (chunk - off) : (uint64_t)kFlagBlock;
        const uint8_t* fl = fl_buf;
        if (one_trip) fl = h->h_careful + kCarefulCountsBytes + off;
        else {
            e = hipMemcpy(fl_buf, h->d_flags.as<uint8_t>() + off, cnt, hipMemcpyDeviceToHost);
            if (e != hipSuccess) { rc = fail(h, NFAGG_EDEVICE, "flag copy failed: %s", hipGetErrorString(e)); break; }
        }
        uint64_t split = off;
        for (uint64_t k = 0; k < cnt; k++) {
            if (fl[k]) { before++; if (before == want) { split = off + k; break; } }
        }
        if (split > 0 && (rc = launch_ingest_profiled(h, d, split, seq0)) != NFAGG_OK) break;
        h->epoch_seq += split; consumed += split;
        h->stats.records_ingested += split;
        h->live = maxe > h->live ? maxe : h->live;   // len(entries) == maxEntries now
        h->live_ub = h->live + (total_new - room);   // = the device's n_live: the chunk's new keys all hold a slot
        h->counters_exact = true;
        h->epoch_len_hint = h->epoch_seq > 1 ? h->epoch_seq : 1;
        h->must_evict = true;
        h->split_seq = seq0 + split;
        rc = NFAGG_FULL;
        break;
    }
    if (consumed_out) *consumed_out = consumed;
    return rc;
}

// ---- sub-flow tables (kernel-dedup mode of a local-fold rank): the join that ends an epoch (nfagg_dedup_join.hip) ----------------
// J: a flow-keyed table of the ordinary kernel-dedup layout, as large as the sub-flow table (a join claims at most one slot per
// live sub-flow). It lives from the first eviction on and is emptied, like the main table, by its epoch tag.
int subflow_join_table(nfagg_handle* h) {
    TableView& J = h->jv;
    if (J.ctr) return NFAGG_OK;
    const uint64_t slots = h->slots;
    TableMem& M = h->jtable;                                    // (a call that failed half way leaves what it allocated, the next one completes it)
    if (!M.hot) HIP_TRY(h, M.hot.alloc(slots * sizeof(SlotHot)));
    if (!M.cold) HIP_TRY(h, M.cold.alloc(slots * sizeof(SlotCold)));
    if (!M.aux) HIP_TRY(h, M.aux.alloc(slots * sizeof(SlotAux)));
    if (!M.live_list) HIP_TRY(h, M.live_list.alloc(slots * sizeof(uint32_t)));
    if (!h->jctr_mirror) HIP_TRY(h, h->jctr_mirror.alloc(sizeof(DevCounters)));
    h->h_jctr = h->jctr_mirror.as<DevCounters>();
    J.hot = M.hot.as<SlotHot>(); J.cold = M.cold.as<SlotCold>(); J.aux = M.aux.as<SlotAux>(); J.live_list = M.live_list.as<uint32_t>();
    HIP_TRY(h, M.ctr.alloc(sizeof(DevCounters)));
    DevCounters* c = M.ctr.as<DevCounters>();
    hipError_t e = hipMemsetAsync(c, 0, sizeof(DevCounters), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(J.hot, 0, slots * sizeof(SlotHot), h->stream);       // the tags: every slot free
    if (e != hipSuccess) { M.ctr.reset(); return fail(h, NFAGG_EDEVICE, "join table: %s", hipGetErrorString(e)); }
    J.mask = slots - 1; J.claim_limit = h->tv.claim_limit; J.epoch_bits = 1ull << 48;
    J.n_shards = 1; J.shard_id = 0; J.defer_claims = 0; J.subflow = 0;
    J.ctr = c;                                                  // last: marks the table as complete
    h->stats.table_bytes += slots * (sizeof(SlotHot) + sizeof(SlotCold) + sizeof(SlotAux));
    return NFAGG_OK;
}

// J's slots belong to a past epoch from now on (nothing is written); its counters are reset by the launches that emptied it
int subflow_join_table_next_epoch(nfagg_handle* h) {
    uint64_t next_epoch = (h->jv.epoch_bits >> 48) + 1;
    if (next_epoch > 0xFFFFull) {
        HIP_TRY(h, hipMemsetAsync(h->jv.hot, 0, h->slots * sizeof(SlotHot), h->stream));
        next_epoch = 1;
    }
    h->jv.epoch_bits = next_epoch << 48;
    return NFAGG_OK;
}

// A join that was made and not delivered (the caller's buffer was too small) is void once the table changes again.
int subflow_join_discard(nfagg_handle* h) {
    if (!h->join.dirty) { h->join.valid = false; return NFAGG_OK; }      // (dirty without valid: a join that failed part-way)
    h->join.valid = false; h->join.dirty = false;
    const hipError_t e = launch_reset_counters(h->jv, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "join table reset failed: %s", hipGetErrorString(e));
    return subflow_join_table_next_epoch(h);
}

// Join the live sub-flows that (n_shards, shard_id) owns (n_shards = 1: all of them) into J. Synchronises; h->join holds the outcome.
int subflow_join(nfagg_handle* h, uint32_t n_shards, uint32_t shard_id) {
    int rc;
    if (h->join.valid && h->join.n_shards == n_shards && h->join.shard_id == shard_id) return NFAGG_OK;
    if ((rc = subflow_join_discard(h)) != NFAGG_OK) return rc;
    if ((rc = refresh_counters(h)) != NFAGG_OK) return rc;
    if (h->h_ctr->aborted) return fail(h, NFAGG_EDEVICE, "table too small for the flows this shard owns (claims refused while merging)");
    const uint64_t claimed = h->h_ctr->n_live;
    if ((rc = subflow_join_table(h)) != NFAGG_OK) return rc;
    if ((rc = h->d_join.ensure(h, (size_t)claimed * sizeof(uint32_t) + 16)) != NFAGG_OK) return rc;
    const uint64_t seq_limit = h->must_evict ? h->split_seq - h->seq_origin : ~0ull;
    h->join.dirty = true;
    const hipError_t e = launch_subflow_join(h->tv, h->jv, claimed, seq_limit, n_shards, shard_id, h->d_join.as<uint32_t>(), h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "sub-flow join launch failed: %s", hipGetErrorString(e));
    HIP_TRY(h, hipMemcpyAsync(h->h_jctr, h->jv.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->h_jctr->error || h->h_jctr->aborted)
        return fail(h, NFAGG_EDEVICE, "sub-flow join bailed out (code %u, aborted %u)", h->h_jctr->error, h->h_jctr->aborted);
    h->join.valid = true; h->join.n_shards = n_shards; h->join.shard_id = shard_id;
    h->join.flows = h->h_jctr->n_live; h->join.claimed = claimed;
    return NFAGG_OK;
}

}  // namespace nfagg

// The NUMA node a device hangs off: /sys/bus/pci/devices/<domain:bus:dev.fn>/numa_node (-1: unknown / not a NUMA host).
static int device_numa_node(int device) {
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char* c = bdf; *c; c++) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
    FILE* f = fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

// First handle of the process: the copy workers, bound next to its GPU. Later handles (other GPUs of a group) share them.
static void host_pool_for_device(int device) {
    static std::once_flag once;
    std::call_once(once, [device] { (void)HostPool::get().configure(0, device_numa_node(device), /*explicit_call=*/false); });
}

// ---- the C ABI (declared extern "C" in include/nfagg.h)

uint32_t nfagg_abi_version(void) { return NFAGG_ABI_VERSION; }

const char* nfagg_last_error(const nfagg_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int nfagg_create(const nfagg_config* cfg_in, nfagg_handle** out) {
    if (!cfg_in || !out) return fail(nullptr, NFAGG_EINVAL, "null argument");
    if (cfg_in->struct_size != sizeof(nfagg_config))
        return fail(nullptr, NFAGG_EINVAL, "nfagg_config.struct_size %u != %zu (ABI mismatch)", cfg_in->struct_size, sizeof(nfagg_config));
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, NFAGG_ENODEV, "no HIP device available (%s); libnfagg has no CPU path",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    nfagg_config cfg = *cfg_in;
    if (cfg.device < 0 || cfg.device >= ndev) return fail(nullptr, NFAGG_EINVAL, "device %d out of range (0..%d)", cfg.device, ndev - 1);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg.device) != hipSuccess) return fail(nullptr, NFAGG_ENODEV, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, NFAGG_ENODEV, "device %d is %s; libnfagg is built for gfx950 (MI355X) only", cfg.device, prop.gcnArchName);
    if (cfg.max_entries == 0) cfg.max_entries = 5000;   // CACHE_MAX_FLOWS default (pkg/config/config.go:146)
    if (cfg.mode != NFAGG_MODE_ACCOUNTER && cfg.mode != NFAGG_MODE_KERNEL_DEDUP)
        return fail(nullptr, NFAGG_EINVAL, "unknown mode %u", cfg.mode);
    if (!ingest_variant_supported((int)cfg.ingest_variant, kDiagBuild))
        return fail(nullptr, NFAGG_EINVAL, "ingest_variant %u is not part of this build (phase-timing builds live in libnfagg_diag.so)", cfg.ingest_variant);
    if (cfg.cm_depth == 0) cfg.cm_depth = 4;
    if (cfg.cm_log2_width == 0) cfg.cm_log2_width = 20;
    if (cfg.hll_p == 0) cfg.hll_p = 14;
    if (cfg.cm_depth > 8 || cfg.cm_log2_width < 4 || cfg.cm_log2_width > 28 || cfg.hll_p < 4 || cfg.hll_p > 18)
        return fail(nullptr, NFAGG_EINVAL, "sketch parameters out of range");
    if (cfg.staging_records == 0) cfg.staging_records = 1ull << 20;
    if (cfg.copy_threads > 64) return fail(nullptr, NFAGG_EINVAL, "copy_threads > 64");      // 0: what the copy workers' calibration found best
    if (cfg.n_shards == 0) cfg.n_shards = 1;
    if (cfg.shard_id >= cfg.n_shards) return fail(nullptr, NFAGG_EINVAL, "shard_id %u >= n_shards %u", cfg.shard_id, cfg.n_shards);
    if (cfg.local_fold > 1) return fail(nullptr, NFAGG_EINVAL, "local_fold must be 0 or 1");
    if (cfg.local_fold && cfg.n_shards > 1) return fail(nullptr, NFAGG_EINVAL, "a local-fold rank folds whatever arrives at it: n_shards must be 0 or 1");
    uint64_t slots = cfg.table_log2_slots ? (1ull << cfg.table_log2_slots) : next_pow2(2 * cfg.max_entries);
    if (slots < (1ull << 16)) slots = 1ull << 16;
    if (slots < 2 * cfg.max_entries) return fail(nullptr, NFAGG_EINVAL, "table_log2_slots too small: need >= 2*max_entries slots");
    if (slots > (1ull << 31)) return fail(nullptr, NFAGG_EINVAL, "table larger than 2^31 slots not supported");

    // caller-owned sketch buffers: Count-Min counters are 64-bit words; HyperLogLog registers are ONE BYTE each (round 4) and are
    // raised by a CAS on the 32-bit word that holds them — a buffer that is not 4-byte aligned cannot be updated
    for (int k = 0; k < 2; k++) {
        if (((uintptr_t)cfg.ext_sketch[k] & 7u) != 0) return fail(nullptr, NFAGG_EINVAL, "ext_sketch[%d] (Count-Min, uint64 counters) must be 8-byte aligned", k);
        if (((uintptr_t)cfg.ext_sketch[2 + k] & 3u) != 0)
            return fail(nullptr, NFAGG_EINVAL, "ext_sketch[%d] (HyperLogLog: 1 << hll_p registers of one byte each) must be 4-byte aligned", 2 + k);
    }
    nfagg_handle* h = new (std::nothrow) nfagg_handle();
    if (!h) return fail(nullptr, NFAGG_ENOMEM, "out of host memory");
    h->cfg = cfg; h->device = cfg.device; h->slots = slots;
#define CREATE_TRY(expr)                                                                         \
    do {                                                                                         \
        hipError_t e2_ = (expr);                                                                 \
        if (e2_ != hipSuccess) {                                                                 \
            int rc_ = fail(nullptr, (e2_ == hipErrorOutOfMemory) ? NFAGG_ENOMEM : NFAGG_EDEVICE, \
                           "%s failed: %s", #expr, hipGetErrorString(e2_));                      \
            nfagg_destroy(h);                                                                    \
            return rc_;                                                                          \
        }                                                                                        \
    } while (0)
    CREATE_TRY(hipSetDevice(h->device));
    host_pool_for_device(h->device);            // the copy workers: created with the first handle, next to its GPU (nfagg_hostpool.h)
    CREATE_TRY(h->stream.create());
    CREATE_TRY(h->table.hot.alloc(slots * sizeof(SlotHot)));
    CREATE_TRY(h->table.cold.alloc(slots * sizeof(SlotCold)));
    // the live list can transiently hold bogus claims of the careful path: size it by slots
    CREATE_TRY(h->table.live_list.alloc(slots * sizeof(uint32_t)));
    CREATE_TRY(h->table.ctr.alloc(sizeof(DevCounters)));
    h->tv.hot = h->table.hot.as<SlotHot>(); h->tv.cold = h->table.cold.as<SlotCold>();
    h->tv.live_list = h->table.live_list.as<uint32_t>(); h->tv.ctr = h->table.ctr.as<DevCounters>();
    CREATE_TRY(hipMemsetAsync(h->tv.hot, 0, slots * sizeof(SlotHot), h->stream));
    CREATE_TRY(hipMemsetAsync(h->tv.cold, 0, slots * sizeof(SlotCold), h->stream));
    if (cfg.mode == NFAGG_MODE_KERNEL_DEDUP) {
        CREATE_TRY(h->table.aux.alloc(slots * sizeof(SlotAux)));
        h->tv.aux = h->table.aux.as<SlotAux>();
        CREATE_TRY(hipMemsetAsync(h->tv.aux, 0, slots * sizeof(SlotAux), h->stream));
    }
    CREATE_TRY(hipMemsetAsync(h->tv.ctr, 0, sizeof(DevCounters), h->stream));
    CREATE_TRY(h->ctr_mirror.alloc(sizeof(DevCounters)));
    CREATE_TRY(h->careful_mirror.alloc(kCarefulCountsBytes + kCarefulMaxBatch));
    h->h_ctr = h->ctr_mirror.as<DevCounters>(); h->h_careful = h->careful_mirror.as<uint8_t>();
    h->tv.mask = slots - 1; h->tv.n_shards = cfg.n_shards; h->tv.shard_id = cfg.shard_id;
    // a local-fold rank in kernel-dedup mode keys its table by (flow, interface): nfagg_dedup.h, include/nfagg.h (local_fold)
    h->tv.subflow = (cfg.mode == NFAGG_MODE_KERNEL_DEDUP && cfg.local_fold) ? 1u : 0u;
    h->tv.claim_limit = slots / 4 * 3 + 16;   // max_entries <= slots/2 plus a careful chunk <= slots/4 always fit
    h->tv.epoch_bits = 1ull << 48;            // eviction epoch 1; 0 is "never used"
    // pass 2 of the two-pass fold may collect its claims per workgroup (up to 1024 each, 256 workgroups resident) before
    // counting them: only where that many uncounted claims cannot fill the table
    h->tv.defer_claims = slots >= (1ull << 21) ? 1u : 0u;
    // careful path: never let claimed slots exceed 3/4 of the table
    h->careful_chunk = slots / 4;
    if (h->careful_chunk > (1ull << 22)) h->careful_chunk = 1ull << 22;
    CREATE_TRY(h->d_slot_idx.alloc(h->careful_chunk * sizeof(uint32_t)));
    CREATE_TRY(h->d_flags.alloc(h->careful_chunk));
    CREATE_TRY(h->d_block_counts.alloc(((h->careful_chunk + kFlagBlock - 1) / kFlagBlock) * sizeof(uint32_t)));
    for (int b = 0; b < 2; b++) CREATE_TRY(h->stage_free[b].create());
    for (int b = 0; b < 2; b++) CREATE_TRY(h->stage_up[b].create());
    CREATE_TRY(h->copy_stream.create());
    // sketches
    h->sk.cm_depth = cfg.cm_depth; h->sk.cm_log2w = cfg.cm_log2_width; h->sk.hll_p = cfg.hll_p;
    h->sk.flags = cfg.sketch_flags & (NFAGG_SKETCH_CM | NFAGG_SKETCH_HLL);
    if (h->sk.flags & NFAGG_SKETCH_CM) {
        const size_t bytes = ((size_t)cfg.cm_depth << cfg.cm_log2_width) * sizeof(uint64_t);
        for (int k = 0; k < 2; k++) {
            if (cfg.ext_sketch[k]) h->sk.cm[k] = (uint64_t*)cfg.ext_sketch[k];
            else { CREATE_TRY(h->sketch[k].alloc(bytes)); h->sk.cm[k] = h->sketch[k].as<uint64_t>(); CREATE_TRY(hipMemsetAsync(h->sk.cm[k], 0, bytes, h->stream)); }
        }
    }
    if (h->sk.flags & NFAGG_SKETCH_HLL) {
        const size_t bytes = ((size_t)1 << cfg.hll_p);              // uint8_t registers (hll_p >= 4: a multiple of 4 bytes)
        for (int k = 0; k < 2; k++) {
            if (cfg.ext_sketch[2 + k]) h->sk.hll[k] = (uint8_t*)cfg.ext_sketch[2 + k];
            else { CREATE_TRY(h->sketch[2 + k].alloc(bytes)); h->sk.hll[k] = h->sketch[2 + k].as<uint8_t>(); CREATE_TRY(hipMemsetAsync(h->sk.hll[k], 0, bytes, h->stream)); }
        }
    }
    CREATE_TRY(h->d_hist.alloc(65 * sizeof(uint32_t)));
    CREATE_TRY(h->qtail.alloc((kSpillParts + 1) * sizeof(uint32_t)));
    h->tv.spill.qtail = h->qtail.as<uint32_t>();
    CREATE_TRY(hipMemsetAsync(h->tv.spill.qtail, 0, (kSpillParts + 1) * sizeof(uint32_t), h->stream));
    h->tv.spill.ovf_tail = h->tv.spill.qtail + kSpillParts;
    h->tv.spill.error = &h->tv.ctr->error;
    {   // Partition = the TOP 11 bits of the home slot index: the flows one pass-2 workgroup merges live in one 1/2048 of the
        // table (a 2^17-slot window of a 2^28-slot table) instead of all over it, and what is appended to the live list at
        // about the same time comes from the ~256 windows being flushed at that time — table pages stay hot in the TLBs
        // during the flush and during eviction.
        int bits = 0;
        while ((1ull << bits) < slots) bits++;
        h->tv.spill.part_shift = (uint32_t)(bits - 11);
        h->tv.spill.n_parts = kSpillParts;
    }
    CREATE_TRY(hipStreamSynchronize(h->stream));
#undef CREATE_TRY
    h->stats.table_slots = slots;
    h->stats.table_bytes = slots * (sizeof(SlotHot) + sizeof(SlotCold) + (h->tv.aux ? sizeof(SlotAux) : 0));
    *out = h;
    return NFAGG_OK;
}

// Everything the handle holds is an owner (nfagg_handle.h): deleting it frees it.
void nfagg_destroy(nfagg_handle* h) {
    if (!h) return;
    hipSetDevice(h->device);
    for (const Stream* s : {&h->stream, &h->copy_stream, &h->d2h_stream, &h->d2h_small, &h->par.stream}) if (*s) hipStreamSynchronize(*s);
    prof_resolve(h);
    delete h;
}

int nfagg_ingest_device(nfagg_handle* h, const void* d_records, size_t n, size_t* consumed) {
    if (!h || (!d_records && n)) return fail(h, NFAGG_EINVAL, "null argument");
    if (((uintptr_t)d_records & 15u) != 0) return fail(h, NFAGG_EINVAL, "device records must be 16-byte aligned");
    HIP_TRY(h, hipSetDevice(h->device));
    return ingest_device_core(h, d_records, n, consumed);
}

int nfagg::staging_alloc(nfagg_handle* h) {
    if (h->d_stage[1]) return NFAGG_OK;
    const size_t bytes = (size_t)h->cfg.staging_records * kRecordBytes;
    for (int b = 0; b < 2; b++) {
        HIP_TRY(h, h->pinned[b].alloc(bytes));
        HIP_TRY(h, h->d_stage[b].alloc(bytes));
    }
    return NFAGG_OK;
}

// Caller buffer -> pinned staging buffer (and bounce buffer -> caller buffer). One core's memcpy (~28 GB/s) is slower than the PCIe
// link the pinned buffer feeds (~57 GB/s), so large copies are cut into parts for the process's copy workers (nfagg_hostpool.h:
// bound to the GPU's NUMA node, non-temporal stores). threads: cfg.copy_threads — 0 = the number of parts the workers' calibration
// found best on this host, 1 = inline.
void nfagg::staged_copy(void* dst, const void* src, size_t bytes, unsigned threads) {
    if (threads == 1) { memcpy(dst, src, bytes); return; }
    HostPool::get().copy(dst, src, bytes, threads);
}

// Device -> caller buffer (pageable). The data must be complete on the device (the caller synchronised the producing stream).
// Chunks go down into two pinned bounce buffers in turn on a stream of their own; while chunk k travels, chunk k-1 is copied
// out of its bounce buffer by cfg.copy_threads threads — the mirror image of the H2D staging ring.
// Is p page-locked host memory the device can read or write directly (nfagg_host_alloc, hipHostMalloc, hipHostRegister)? Such
// a buffer needs no trip through the library's own pinned buffers: the DMA engine takes it as it is.
bool nfagg::host_is_pinned(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // plain malloc memory: "invalid value"
    return a.type == hipMemoryTypeHost;
}

constexpr size_t kBounceBytes = 16u << 20;
int nfagg::d2h_copy(nfagg_handle* h, void* dst, const void* d_src, size_t bytes) {
    if (bytes == 0) return NFAGG_OK;
    if (bytes < (4u << 20) || host_is_pinned(dst)) {
        // NOT a blocking hipMemcpy: that one runs on the legacy stream, and nfagg_account calls this from a helper thread while the
        // calling thread may be CAPTURING the epoch chain's graph on the handle's stream — the capture was invalidated now and then
        // ("operation failed due to a previous error during capture", once in ~240 soak streams: profiles/r05_soak_account.txt).
        // On a stream of ITS OWN: a copy into pageable memory on d2h_stream left that stream's later page-locked downloads at
        // a third of the link (nfagg_account from page-locked buffers 22.0 -> 28.0 ms, same box: profiles/r05_account_host_pipeline.txt)
        if (!h->d2h_small) HIP_TRY(h, h->d2h_small.create());
        HIP_TRY(h, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, h->d2h_small));
        HIP_TRY(h, hipStreamSynchronize(h->d2h_small));
        return NFAGG_OK;
    }
    if (!h->d2h_stream) HIP_TRY(h, h->d2h_stream.create());
    for (int b = 0; b < 2; b++) {                                // created on first use; a failure part-way is picked up by the next call
        if (!h->h_bounce[b]) HIP_TRY(h, h->h_bounce[b].alloc(kBounceBytes));
        if (!h->bounce_ev[b]) HIP_TRY(h, h->bounce_ev[b].create());
    }
    const size_t n_chunks = (bytes + kBounceBytes - 1) / kBounceBytes;
    for (size_t k = 0; k <= n_chunks; k++) {
        if (k < n_chunks) {
            const size_t off = k * kBounceBytes, len = bytes - off < kBounceBytes ? bytes - off : kBounceBytes;
            HIP_TRY(h, hipMemcpyAsync(h->h_bounce[k & 1].p, (const char*)d_src + off, len, hipMemcpyDeviceToHost, h->d2h_stream));
            HIP_TRY(h, hipEventRecord(h->bounce_ev[k & 1], h->d2h_stream));
        }
        if (k > 0) {
            const size_t off = (k - 1) * kBounceBytes, len = bytes - off < kBounceBytes ? bytes - off : kBounceBytes;
            HIP_TRY(h, hipEventSynchronize(h->bounce_ev[(k - 1) & 1]));
            staged_copy((char*)dst + off, h->h_bounce[(k - 1) & 1].p, len, h->cfg.copy_threads);
        }
    }
    return NFAGG_OK;
}

// How much of a host buffer goes up in one piece. A stream that keeps stopping on "full" (small CACHE_MAX_FLOWS: the reference's
// default is 5000, config.go:146) consumes one epoch per call — about epoch_len_hint records — and what was staged beyond that
// is staged again by the next call: copy what is left of the epoch and a quarter more (a longer epoch simply takes another
// chunk), not a whole staging buffer. Measured at max_entries 5000: 3.6 -> 36 M records/s through nfagg_ingest / nfagg_evict.
size_t nfagg::stage_chunk(const nfagg_handle* h, size_t remaining, size_t cap) {
    size_t m = remaining < cap ? remaining : cap;
    if (h->epoch_len_hint) {
        const uint64_t reach = h->epoch_len_hint + h->epoch_len_hint / 4;
        uint64_t want = reach > h->epoch_seq ? reach - h->epoch_seq : 0;
        if (want < kCarefulMaxBatch) want = kCarefulMaxBatch;
        if (m > want) m = (size_t)want;
    }
    return m;
}

int nfagg_ingest(nfagg_handle* h, const void* records, size_t n, size_t* consumed_out) {
    if (!h || (!records && n)) return fail(h, NFAGG_EINVAL, "null argument");
    if (h->stage_acquired) return fail(h, NFAGG_ESTATE, "a staging buffer is acquired; commit it first");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = staging_alloc(h);
    if (rc != NFAGG_OK) return rc;
    size_t consumed = 0;
    const char* src = static_cast<const char*>(records);
    const size_t cap = (size_t)h->cfg.staging_records;
    const bool pinned_src = host_is_pinned(records);            // page-locked caller buffer: sent up as it is, no host copy
    // ---- the whole call folded optimistically (round 5). A call of several staging buffers into a table it MIGHT fill (live + n >
    // max_entries) used to ask the device for the exact len(entries) before every chunk — a stream synchronisation that also stops
    // the host from copying the next chunk: host copy and upload took turns instead of overlapping (20 M records from pageable
    // memory: 88 ms, 227 M records/s, where the same call into a table that cannot fill ran at the link's 374 M). Here the chunks
    // are folded without a look in between and the proof comes ONCE, after the last: n_live <= max_entries and no refused claim
    // means no record of the call found the map full (account.go:85; DESIGN.md §2 "optimistic fold"). Otherwise everything is
    // rolled back (raw copy of the live slots, sketches, counters: taken before the first chunk) and the loop below does it step by step.
    if (n > cap && n <= kMaxFoldChunk && h->epoch_len_hint == 0 && !h->must_evict && !h->exported && !h->tv.subflow && !h->ext_sequenced) {
        if (!h->mirror_fresh && (rc = refresh_counters(h)) != NFAGG_OK) return rc;
        bool blocked = false;
        if (h->live + n > h->cfg.max_entries && (rc = ensure_seq_window(h, n, &blocked)) == NFAGG_OK && !blocked) {
            OptState st;
            if ((rc = opt_begin(h, st)) != NFAGG_OK) return rc;
            size_t off = 0;
            while (off < n && rc == NFAGG_OK) {
                const size_t m = (n - off) < cap ? (n - off) : cap;
                const int b = h->stage_next;
                HIP_TRY(h, hipEventSynchronize(h->stage_free[b]));
                const void* up = src + off * kRecordBytes;
                if (!pinned_src) { staged_copy(h->pinned[b].p, up, m * kRecordBytes, h->cfg.copy_threads); up = h->pinned[b].p; }
                HIP_TRY(h, hipMemcpyAsync(h->d_stage[b].p, up, m * kRecordBytes, hipMemcpyHostToDevice, h->copy_stream));
                HIP_TRY(h, hipEventRecord(h->stage_up[b], h->copy_stream));
                HIP_TRY(h, hipStreamWaitEvent(h->stream, h->stage_up[b], 0));
                rc = launch_ingest_profiled(h, h->d_stage[b].p, m, st.seq0 + off);
                HIP_TRY(h, hipEventRecord(h->stage_free[b], h->stream));
                h->stage_next ^= 1;
                off += m;
            }
            if (rc != NFAGG_OK) return rc;
            if ((rc = refresh_counters(h)) != NFAGG_OK) return rc;       // the one wait of the call
            h->stats.optimistic_folds++;
            st.n_after = h->h_ctr->n_live;
            if (!h->h_ctr->aborted && st.n_after <= h->cfg.max_entries) {
                opt_commit(h, st, n);
                if (pinned_src) HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
                if (consumed_out) *consumed_out = n;
                return NFAGG_OK;
            }
            if ((rc = opt_rollback(h, st)) != NFAGG_OK) return rc;       // some record found the map full: step by step, below
        } else if (rc != NFAGG_OK) return rc;
    }
    // pinned ring, double buffered: the CPU fills buffer b+1 while the GPU
    // copies/folds buffer b (tracer_ringbuf.go:112-134 forwards one record at a time)
    while (consumed < n) {
        const size_t m = stage_chunk(h, n - consumed, cap);
        const int b = h->stage_next;
        HIP_TRY(h, hipEventSynchronize(h->stage_free[b]));
        const void* up = src + consumed * kRecordBytes;
        if (!pinned_src) { staged_copy(h->pinned[b].p, up, m * kRecordBytes, h->cfg.copy_threads); up = h->pinned[b].p; }
        // the copy runs on its own stream: the fold of the previous chunk (other buffer) is still busy on h->stream
        HIP_TRY(h, hipMemcpyAsync(h->d_stage[b].p, up, m * kRecordBytes, hipMemcpyHostToDevice, h->copy_stream));
        HIP_TRY(h, hipEventRecord(h->stage_up[b], h->copy_stream));
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->stage_up[b], 0));
        size_t c = 0;
        rc = ingest_device_core(h, h->d_stage[b].p, m, &c);
        HIP_TRY(h, hipEventRecord(h->stage_free[b], h->stream));
        h->stage_next ^= 1;
        consumed += c;
        if (rc != NFAGG_OK) break;
    }
    if (pinned_src) HIP_TRY(h, hipStreamSynchronize(h->copy_stream));   // the caller's buffer is its own again when the call returns
    if (consumed_out) *consumed_out = consumed;
    return rc;
}

int nfagg_staging_acquire(nfagg_handle* h, void** buf, size_t* capacity_records) {
    if (!h || !buf) return fail(h, NFAGG_EINVAL, "null argument");
    if (h->stage_acquired) return fail(h, NFAGG_ESTATE, "staging buffer already acquired");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = staging_alloc(h);
    if (rc != NFAGG_OK) return rc;
    const int b = h->stage_next;
    HIP_TRY(h, hipEventSynchronize(h->stage_free[b]));
    *buf = h->pinned[b].p;
    if (capacity_records) *capacity_records = (size_t)h->cfg.staging_records;
    h->stage_acquired = true;
    return NFAGG_OK;
}

int nfagg_staging_commit(nfagg_handle* h, size_t n, size_t* consumed) {
    if (!h) return NFAGG_EINVAL;
    if (!h->stage_acquired) return fail(h, NFAGG_ESTATE, "no staging buffer acquired");
    if (n > h->cfg.staging_records) return fail(h, NFAGG_EINVAL, "n exceeds staging capacity");
    HIP_TRY(h, hipSetDevice(h->device));
    const int b = h->stage_next;
    h->stage_acquired = false;
    HIP_TRY(h, hipMemcpyAsync(h->d_stage[b].p, h->pinned[b].p, n * kRecordBytes, hipMemcpyHostToDevice, h->copy_stream));
    HIP_TRY(h, hipEventRecord(h->stage_up[b], h->copy_stream));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->stage_up[b], 0));
    int rc = ingest_device_core(h, h->d_stage[b].p, n, consumed);
    HIP_TRY(h, hipEventRecord(h->stage_free[b], h->stream));
    h->stage_next ^= 1;
    return rc;
}

int nfagg_len(nfagg_handle* h, uint64_t* entries) {
    if (!h || !entries) return fail(h, NFAGG_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = refresh_counters(h);
    if (rc != NFAGG_OK) return rc;
    *entries = h->live;
    return NFAGG_OK;
}

// The table itself is never cleared: the slots of the flows that just left simply belong to a past epoch tag.
// Tags hold 16 bits of epoch; when they wrap (every 65 535 bumps) the tags are cleared once.
static int bump_epoch(nfagg_handle* h) {
    uint64_t next_epoch = (h->tv.epoch_bits >> 48) + 1;
    if (next_epoch > 0xFFFFull) {
        HIP_TRY(h, hipMemsetAsync(h->tv.hot, 0, h->slots * sizeof(SlotHot), h->stream));
        next_epoch = 1;
    }
    h->tv.epoch_bits = next_epoch << 48;
    return NFAGG_OK;
}

// The bookkeeping that ends an eviction epoch (the kernels have been launched; the device counters are reset by them).
static int finish_epoch(nfagg_handle* h, int reason, uint64_t flows) {
    h->last_epoch_flows = h->tv.subflow ? h->join.claimed : flows;
    h->stats.evictions[reason]++;
    h->stats.evicted_flows[reason] += flows;
    h->epoch_seq = 0; h->seq_origin = 0; h->live = 0; h->live_ub = 0; h->must_evict = false; h->split_seq = 0; h->exported = false;
    h->counters_exact = true;          // k_reset_after_evict left n_live = 0
    h->epoch_unclustered = false;
    h->abort_cap = 0;                  // one batch with more new keys than the table takes does not cap the chunks of later epochs
    return bump_epoch(h);
}

// Accounter.evict (account.go:102-124) for a sub-flow table: the join (nfagg_dedup_join.hip) of the sub-flows that (n_shards,
// shard_id) owns into the flow-keyed table, then k_evict_dedup over that. NFAGG_TRUNCATED (nothing evicted; the join is kept for
// the repeated call) when cap is too small.
static int subflow_evict(nfagg_handle* h, int reason, uint32_t n_shards, uint32_t shard_id, void* out, bool out_is_device, size_t cap, size_t* n_out) {
    int rc;
    *n_out = 0;
    if (!h->counters_exact && (rc = refresh_counters(h)) != NFAGG_OK) return rc;
    if (reason == NFAGG_REASON_TIMEOUT && h->live_ub == 0 && !h->exported) return NFAGG_OK;      // account.go:64-66
    if ((rc = subflow_join(h, n_shards, shard_id)) != NFAGG_OK) return rc;
    const uint64_t flows = h->join.flows;
    *n_out = (size_t)flows;
    if (flows > cap) return NFAGG_TRUNCATED;
    if (flows && !out) return fail(h, NFAGG_EINVAL, "null output buffer");
    void* d_out = out;
    if (!out_is_device) {
        if ((rc = h->d_evict.ensure(h, (size_t)flows * kRecordBytes + 16)) != NFAGG_OK) return rc;
        d_out = h->d_evict.p;
    }
    HIP_TRY(h, hipMemsetAsync(&h->jv.ctr->n_out, 0, sizeof(unsigned long long), h->stream));
    EventPair ep{};
    if (h->cfg.profile) prof_begin(h, ep, 1);
    hipError_t e = launch_evict_dedup(h->jv, flows, ~0ull, d_out, h->stream);      // leaves J's counters reset
    if (e == hipSuccess) e = launch_reset_counters(h->tv, h->stream);
    if (h->cfg.profile) prof_end(h, ep);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "evict launch failed: %s", hipGetErrorString(e));
    HIP_TRY(h, hipMemcpyAsync(h->h_jctr, h->jv.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!out_is_device && flows && (rc = d2h_copy(h, out, h->d_evict.p, (size_t)flows * kRecordBytes)) != NFAGG_OK) return rc;
    h->mirror_fresh = false;
    if (h->h_jctr->error) return fail(h, NFAGG_EDEVICE, "sub-flow join table kernel bailed out (code %u)", h->h_jctr->error);
    if (h->h_jctr->n_out != flows)
        return fail(h, NFAGG_EDEVICE, "evict wrote %llu records, expected %llu", (unsigned long long)h->h_jctr->n_out, (unsigned long long)flows);
    h->join.valid = false; h->join.dirty = false;                 // launch_evict_dedup left J's counters reset; its slots expire with the tag
    if ((rc = subflow_join_table_next_epoch(h)) != NFAGG_OK) return rc;
    return finish_epoch(h, reason, flows);
}

int nfagg::evict_core(nfagg_handle* h, int reason, void* out, bool out_is_device, size_t cap, size_t* n_out) {
    if (!h || !n_out || reason < 0 || reason > 2) return fail(h, NFAGG_EINVAL, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = NFAGG_OK;
    if (h->exported) return fail(h, NFAGG_ESTATE, "partials were exported from / merged into this table: evict it with nfagg_evict_owned_device");
    if (h->tv.subflow) return subflow_evict(h, reason, 1, 0, out, out_is_device, cap, n_out);
    if (!h->counters_exact && (rc = refresh_counters(h)) != NFAGG_OK) return rc;
    const uint64_t legit = h->live;
    const uint64_t claimed = h->live_ub;          // = the device's n_live (counters_exact)
    *n_out = (size_t)legit;
    if (legit > cap) return NFAGG_TRUNCATED;
    if (legit && !out) return fail(h, NFAGG_EINVAL, "null output buffer");
    if (reason == NFAGG_REASON_TIMEOUT && legit == 0 && claimed == 0) return NFAGG_OK;  // account.go:64-66
    void* d_out = out;
    if (!out_is_device) {
        if ((rc = h->d_evict.ensure(h, (size_t)legit * kRecordBytes + 16)) != NFAGG_OK) return rc;
        d_out = h->d_evict.p;
    }
    HIP_TRY(h, hipMemsetAsync(&h->tv.ctr->n_out, 0, sizeof(unsigned long long), h->stream));
    // large table: visit the claimed slots in address order (see launch_sort_slots)
    TableView tv = h->tv;
    // ... unless every batch of the epoch went through the two-pass fold: its pass-2 workgroups claim slots partition by
    // partition (partition = top bits of the slot index), the live list is clustered already and the sort does not pay
    // (0.27 ms unsorted against 0.40 ms sorted per 1 M flows of a 64 GiB table; 0.49 ms before either).
    bool sort_slots = claimed >= (1u << 16) && h->slots >= (1ull << 24) && claimed < (1ull << 31) && h->epoch_unclustered;
    size_t temp_bytes = 0;
    if (sort_slots) {
        int bits = 0;
        while ((1ull << bits) < h->slots) bits++;
        h->sort_bits = bits;
        hipError_t es = launch_sort_slots(h->tv.live_list, nullptr, claimed, bits, nullptr, &temp_bytes, h->stream);
        if (es != hipSuccess) return fail(h, NFAGG_EDEVICE, "sort size query failed: %s", hipGetErrorString(es));
        if ((rc = h->sort_live.ensure(h, claimed * sizeof(uint32_t))) != NFAGG_OK) return rc;
        if ((rc = h->sort_tmp.ensure(h, temp_bytes + 16)) != NFAGG_OK) return rc;
    }
    EventPair ep{};
    if (h->cfg.profile) prof_begin(h, ep, 1);
    if (sort_slots) {
        hipError_t es = launch_sort_slots(h->tv.live_list, h->sort_live.as<uint32_t>(), claimed, h->sort_bits, h->sort_tmp.p, &temp_bytes, h->stream);
        if (es != hipSuccess) return fail(h, NFAGG_EDEVICE, "slot sort failed: %s", hipGetErrorString(es));
        tv.live_list = h->sort_live.as<uint32_t>();
    }
    hipError_t e = launch_evict(tv, claimed, h->must_evict ? h->split_seq - h->seq_origin : ~0ull, d_out, h->stream);
    if (h->cfg.profile) prof_end(h, ep);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "evict launch failed: %s", hipGetErrorString(e));
    // counters and (host variant) the records come back in stream order behind the kernel: one wait for both
    HIP_TRY(h, hipMemcpyAsync(h->h_ctr, h->tv.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (!out_is_device && legit && (rc = d2h_copy(h, out, h->d_evict.p, (size_t)legit * kRecordBytes)) != NFAGG_OK) return rc;
    h->mirror_fresh = true;
    if (h->h_ctr->error)
        return fail(h, NFAGG_EDEVICE, "flow table kernel bailed out (code %u: 1 = probe overflow / table too small, 2 = claim spin limit, 5 = spill overflow list full, 6 = claimed slot without a record, 7 = partial of another shard merged)", h->h_ctr->error);
    if (h->h_ctr->n_out != legit)
        return fail(h, NFAGG_EDEVICE, "evict wrote %llu records, expected %llu", (unsigned long long)h->h_ctr->n_out, (unsigned long long)legit);
    h->stats.records_skipped = h->h_ctr->n_skipped;
    h->stats.records_bypassed = h->h_ctr->n_bypassed;
    if (h->h_ctr->max_probe > h->stats.max_probe) h->stats.max_probe = h->h_ctr->max_probe;
    return finish_epoch(h, reason, legit);
}

int nfagg_evict(nfagg_handle* h, int reason, void* out, size_t cap, size_t* n_out) {
    return evict_core(h, reason, out, false, cap, n_out);
}

int nfagg_evict_device(nfagg_handle* h, int reason, void* d_out, size_t cap, size_t* n_out) {
    if (d_out && ((uintptr_t)d_out & 15u)) return fail(h, NFAGG_EINVAL, "device output must be 16-byte aligned");
    return evict_core(h, reason, d_out, true, cap, n_out);
}

// ---------------------------------------------------------------- local fold across GPUs: partials (nfagg_combine.hip)
// The three steps of the local-fold tick as handle calls. The one-process group (nfagg_api_group.hip) and one-process-per-GPU
// ranks (bench.py --gpus N: exchange with an RCCL all-to-all) run the same code.
static int partials_scratch(nfagg_handle* h) {
    int rc = h->d_exp.ensure(h, 136 * sizeof(unsigned long long));
    if (rc != NFAGG_OK) return rc;
    if (!h->exp_mirror) HIP_TRY(h, h->exp_mirror.alloc(136 * sizeof(unsigned long long)));
    h->h_exp = h->exp_mirror.as<unsigned long long>();
    return NFAGG_OK;
}

// counts[o] (host, n_shards words) = flows of segment o; *n_out = their sum. NFAGG_TRUNCATED (nothing written, state unchanged)
// when cap is too small. The partials are complete in d_out when the call returns.
int nfagg::partials_export_core(nfagg_handle* h, uint32_t n_shards, uint32_t self_shard, void* d_out, size_t cap, uint64_t* counts,
                                size_t* n_out) {
    if (!h || !counts || !n_out) return fail(h, NFAGG_EINVAL, "null argument");
    if (n_shards == 0 || n_shards > 64) return fail(h, NFAGG_EINVAL, "n_shards must be in [1, 64]");
    if (h->cfg.mode != NFAGG_MODE_ACCOUNTER && !h->tv.subflow)
        return fail(h, NFAGG_EINVAL, "partials need NFAGG_MODE_ACCOUNTER, or NFAGG_MODE_KERNEL_DEDUP on a handle created with nfagg_config.local_fold (flow-keyed kernel-dedup slots do not merge across tables)");
    if (h->cfg.n_shards > 1) return fail(h, NFAGG_ESTATE, "a handle that filters its input by shard (n_shards > 1) holds no other shard's flows");
    if (d_out && ((uintptr_t)d_out & 63u)) return fail(h, NFAGG_EINVAL, "partials buffer must be 64-byte aligned");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = partials_scratch(h);
    if (rc != NFAGG_OK) return rc;
    if ((rc = refresh_counters(h)) != NFAGG_OK) return rc;
    const uint64_t claimed = h->h_ctr->n_live;
    const uint64_t seq_limit = h->must_evict ? h->split_seq - h->seq_origin : ~0ull;
    unsigned long long* d_counts = h->d_exp.as<unsigned long long>();
    unsigned long long* d_cursor = d_counts + 64;
    hipError_t e = launch_export_count(h->tv, claimed, seq_limit, n_shards, self_shard, d_counts, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "partials count launch failed: %s", hipGetErrorString(e));
    HIP_TRY(h, hipMemcpyAsync(h->h_exp, d_counts, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    uint64_t total = 0;
    for (uint32_t o = 0; o < n_shards; o++) { counts[o] = h->h_exp[o]; h->h_exp[64 + o] = total; total += counts[o]; }
    *n_out = (size_t)total;
    if (total > cap) return NFAGG_TRUNCATED;
    if (total && !d_out) return fail(h, NFAGG_EINVAL, "null partials buffer");
    if (total) {
        HIP_TRY(h, hipMemcpyAsync(d_cursor, h->h_exp + 64, 64 * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
        e = launch_export_scatter(h->tv, claimed, seq_limit, n_shards, self_shard, d_cursor, d_out, h->stream);
        if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "partials export launch failed: %s", hipGetErrorString(e));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (self_shard < n_shards && n_shards > 1) h->exported = true;       // other shards' flows are on their way to their owners
    return NFAGG_OK;
}

// Asynchronous (the handle's stream); d_partials must stay valid until the handle synchronises.
int nfagg::partials_merge_core(nfagg_handle* h, uint32_t n_shards, uint32_t shard_id, const void* d_partials, size_t n) {
    if (!h || (n && !d_partials)) return fail(h, NFAGG_EINVAL, "null argument");
    if (n_shards == 0 || n_shards > 64 || shard_id >= n_shards) return fail(h, NFAGG_EINVAL, "bad shard (n_shards in [1, 64], shard_id < n_shards)");
    if (h->cfg.mode != NFAGG_MODE_ACCOUNTER && !h->tv.subflow) return fail(h, NFAGG_EINVAL, "partials need NFAGG_MODE_ACCOUNTER or nfagg_config.local_fold");
    if ((uintptr_t)d_partials & 15u) return fail(h, NFAGG_EINVAL, "partials buffer must be 16-byte aligned");
    if (n == 0) return NFAGG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    { const int rcj = subflow_join_discard(h); if (rcj != NFAGG_OK) return rcj; }
    TableView tv = h->tv;
    tv.n_shards = n_shards; tv.shard_id = shard_id;
    h->counters_exact = false; h->mirror_fresh = false;                  // the merge claims slots
    h->exported = true;                                                  // merged state: only the eviction may follow
    const hipError_t e = launch_merge_raw(tv, d_partials, n, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "partials merge launch failed: %s", hipGetErrorString(e));
    return NFAGG_OK;
}

// *owned = flows of this table that (n_shards, shard_id) owns — what evict_owned_core will write. Synchronises; reports
// claims refused by a merge.
int nfagg::owned_count_core(nfagg_handle* h, uint32_t n_shards, uint32_t shard_id, uint64_t* owned, uint64_t* claimed_out) {
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    if (h->tv.subflow) {                                         // flows, not sub-flows: known after the join (kept for the eviction)
        if ((rc = subflow_join(h, n_shards, shard_id)) != NFAGG_OK) return rc;
        *owned = h->join.flows;
        if (claimed_out) *claimed_out = h->join.claimed;
        return NFAGG_OK;
    }
    rc = partials_scratch(h);
    if (rc != NFAGG_OK) return rc;
    if ((rc = refresh_counters(h)) != NFAGG_OK) return rc;
    if (h->h_ctr->aborted) return fail(h, NFAGG_EDEVICE, "table too small for the flows this shard owns (claims refused while merging)");
    const uint64_t claimed = h->h_ctr->n_live;
    TableView tv = h->tv;
    tv.n_shards = n_shards; tv.shard_id = shard_id;
    unsigned long long* d_owned = h->d_exp.as<unsigned long long>() + 128;
    const hipError_t e = launch_count_owned(tv, claimed, h->must_evict ? h->split_seq - h->seq_origin : ~0ull, d_owned, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "owned count launch failed: %s", hipGetErrorString(e));
    HIP_TRY(h, hipMemcpyAsync(h->h_exp + 128, d_owned, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *owned = h->h_exp[128];
    if (claimed_out) *claimed_out = claimed;
    return NFAGG_OK;
}

int nfagg::evict_owned_core(nfagg_handle* h, int reason, uint32_t n_shards, uint32_t shard_id, void* d_out, size_t cap, size_t* n_out) {
    if (!h || !n_out || reason < 0 || reason > 2) return fail(h, NFAGG_EINVAL, "bad argument");
    if (n_shards == 0 || n_shards > 64 || shard_id >= n_shards) return fail(h, NFAGG_EINVAL, "bad shard (n_shards in [1, 64], shard_id < n_shards)");
    if (h->cfg.mode != NFAGG_MODE_ACCOUNTER && !h->tv.subflow) return fail(h, NFAGG_EINVAL, "partials need NFAGG_MODE_ACCOUNTER or nfagg_config.local_fold");
    if (d_out && ((uintptr_t)d_out & 15u)) return fail(h, NFAGG_EINVAL, "device output must be 16-byte aligned");
    if (h->tv.subflow) { HIP_TRY(h, hipSetDevice(h->device)); return subflow_evict(h, reason, n_shards, shard_id, d_out, true, cap, n_out); }
    uint64_t owned = 0, claimed = 0;
    int rc = owned_count_core(h, n_shards, shard_id, &owned, &claimed);
    if (rc != NFAGG_OK) return rc;
    *n_out = (size_t)owned;
    if (owned > cap) return NFAGG_TRUNCATED;
    if (owned && !d_out) return fail(h, NFAGG_EINVAL, "null output buffer");
    if (reason == NFAGG_REASON_TIMEOUT && claimed == 0 && !h->exported) return NFAGG_OK;      // account.go:64-66
    HIP_TRY(h, hipMemsetAsync(&h->tv.ctr->n_out, 0, sizeof(unsigned long long), h->stream));
    TableView tv = h->tv;
    tv.n_shards = n_shards; tv.shard_id = shard_id;
    EventPair ep{};
    if (h->cfg.profile) prof_begin(h, ep, 1);
    const hipError_t e = launch_evict_filtered(tv, claimed, h->must_evict ? h->split_seq - h->seq_origin : ~0ull, d_out, h->stream);
    if (h->cfg.profile) prof_end(h, ep);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "evict launch failed: %s", hipGetErrorString(e));
    HIP_TRY(h, hipMemcpyAsync(h->h_ctr, h->tv.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->h_ctr->n_out != owned)
        return fail(h, NFAGG_EDEVICE, "evict wrote %llu records, expected %llu", (unsigned long long)h->h_ctr->n_out, (unsigned long long)owned);
    return finish_epoch(h, reason, owned);
}

int nfagg_partials_export_device(nfagg_handle* h, uint32_t n_shards, uint32_t self_shard, void* d_out, size_t cap, uint64_t* counts, size_t* n_out) {
    return partials_export_core(h, n_shards, self_shard, d_out, cap, counts, n_out);
}

int nfagg_partials_merge_device(nfagg_handle* h, uint32_t n_shards, uint32_t shard_id, const void* d_partials, size_t n) {
    return partials_merge_core(h, n_shards, shard_id, d_partials, n);
}

int nfagg_evict_owned_device(nfagg_handle* h, int reason, uint32_t n_shards, uint32_t shard_id, void* d_out, size_t cap, size_t* n_out) {
    return evict_owned_core(h, reason, n_shards, shard_id, d_out, cap, n_out);
}

size_t nfagg_partial_bytes(const nfagg_handle* h) { return (h && h->tv.subflow) ? kPartialBytesDedup : kPartialBytes; }

int nfagg_set_sequence(nfagg_handle* h, uint64_t next_seq) {
    if (!h) return NFAGG_EINVAL;
    if (next_seq < h->epoch_seq) return fail(h, NFAGG_EINVAL, "sequence numbers do not go backwards inside an epoch (%llu < %llu)",
                                             (unsigned long long)next_seq, (unsigned long long)h->epoch_seq);
    h->epoch_seq = next_seq;
    h->ext_sequenced = true;                                    // other tables number their records in the same space
    return NFAGG_OK;
}

// ---- the sequence window of tables that share ONE numbering (local fold across GPUs) ---------------------------------
// Such a table cannot rebase its tags on its own (nfagg_rebase.hip): the flows are first brought together at their owners —
// every table exports ALL its flows as partials grouped by owner (nfagg_partials_export_device with NFAGG_SHARD_NONE),
// empties itself (window_clear_core: the epoch tag, nothing is written), takes in what it owns (partials_merge_core, its own
// segment included) and rebases the single copy it now holds (window_finish_core). No flow leaves the epoch, the sketches are
// not touched; len(entries) of a table becomes the number of flows it owns.
int nfagg::window_clear_core(nfagg_handle* h) {
    if (h->must_evict) return fail(h, NFAGG_ESTATE, "an eviction on full is pending");
    HIP_TRY(h, hipSetDevice(h->device));
    const hipError_t e = launch_reset_counters(h->tv, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "counter reset launch failed: %s", hipGetErrorString(e));
    h->live = h->live_ub = 0; h->counters_exact = true; h->mirror_fresh = false;
    h->epoch_unclustered = false; h->exported = false;
    return bump_epoch(h);
}

int nfagg::window_finish_core(nfagg_handle* h, uint64_t next_seq) {
    if (next_seq < h->epoch_seq || next_seq < rebase_keep()) return fail(h, NFAGG_EINVAL, "window restart: next sequence number %llu below what the handle has reached",
                                                                         (unsigned long long)next_seq);
    HIP_TRY(h, hipSetDevice(h->device));
    hipError_t e = launch_finalize(h->tv, nullptr, 0, 0, h->stream);          // the merges copied the identity dwords: everything is finalized
    if (e == hipSuccess) e = launch_rebase(h->tv, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "window restart launch failed: %s", hipGetErrorString(e));
    h->epoch_seq = next_seq; h->seq_origin = next_seq - rebase_keep();
    h->exported = false; h->counters_exact = false; h->mirror_fresh = false;
    h->stats.sequence_rebases++;
    const int rc = refresh_counters(h);                                        // len(entries) = the flows this table owns now; reports refused claims
    if (rc != NFAGG_OK) return rc;
    if (h->h_ctr->aborted) return fail(h, NFAGG_EDEVICE, "table too small for the flows this shard owns (claims refused while merging)");
    h->epoch_unclustered = true;
    return NFAGG_OK;
}

int nfagg_window_restart_device(nfagg_handle* h, uint32_t n_shards, uint32_t shard_id, const void* d_partials, size_t n, uint64_t next_seq) {
    if (!h) return NFAGG_EINVAL;
    if (h->tv.subflow) return fail(h, NFAGG_ESTATE, "kernel-dedup mode: the sequence window of a local-fold job does not move (the order between a flow's sub-flows would be lost): evict instead");
    int rc = window_clear_core(h);
    if (rc != NFAGG_OK) return rc;
    if ((rc = partials_merge_core(h, n_shards, shard_id, d_partials, n)) != NFAGG_OK) return rc;
    h->ext_sequenced = true;
    return window_finish_core(h, next_seq);
}

// Page-locked host memory for record / eviction buffers: what nfagg_ingest, nfagg_account and nfagg_evict are handed in such a
// buffer crosses PCIe by DMA straight from / into it (no copy through the library's staging ring).
int nfagg_host_alloc(size_t bytes, void** p) {
    if (!p || bytes == 0) return NFAGG_EINVAL;
    *p = nullptr;
    if (hipHostMalloc(p, bytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return NFAGG_ENOMEM; }
    return NFAGG_OK;
}
void nfagg_host_free(void* p) { if (p) (void)hipHostFree(p); }

int nfagg_host_threads(unsigned threads, int numa_node) {
    if (threads > 64) return NFAGG_EINVAL;
    return (int)HostPool::get().configure(threads, numa_node);
}

int nfagg_host_info(nfagg_host_pool_info* out) {
    if (!out || out->struct_size != sizeof(nfagg_host_pool_info)) return NFAGG_EINVAL;
    HostPool& p = HostPool::get();
    out->workers = p.workers(); out->parts = p.best_parts(); out->numa_node = p.node(); out->bound = p.bound() ? 1u : 0u;
    out->calibrated_gbs = p.calibrated_gbs();
    return NFAGG_OK;
}

int nfagg_device_numa_node(int device) { return device_numa_node(device); }

// pkg/model/record.go:90-97
void nfagg_record_times(int64_t now_unix_ns, uint64_t mono_now_ns, const nfagg_flow_metrics* m,
                        int64_t* time_flow_start_unix_ns, int64_t* time_flow_end_unix_ns) {
    const int64_t start_delta = (int64_t)(mono_now_ns - m->start_mono_time_ts);
    const int64_t end_delta = (int64_t)(mono_now_ns - m->end_mono_time_ts);
    if (time_flow_start_unix_ns) *time_flow_start_unix_ns = (int64_t)((uint64_t)now_unix_ns - (uint64_t)start_delta);
    if (time_flow_end_unix_ns) *time_flow_end_unix_ns = (int64_t)((uint64_t)now_unix_ns - (uint64_t)end_delta);
}

// ---------------------------------------------------------------- misc
uint64_t nfagg_key_hash(const nfagg_flow_id* id) {
    uint64_t w[5];
    memcpy(w, id, 40);
    w[4] &= 0x00ffffffffffffffull;   // byte 39
    return key_hash(w);
}

void nfagg_shard_ids(const void* records, size_t n, uint32_t n_shards, uint32_t* out_shard) {
    const char* p = static_cast<const char*>(records);
    for (size_t i = 0; i < n; i++)
        out_shard[i] = nfagg_shard_of(reinterpret_cast<const nfagg_flow_id*>(p + i * kRecordBytes), n_shards);
}

uint32_t nfagg_shard_of(const nfagg_flow_id* id, uint32_t n_shards) { return shard_of_hash(nfagg_key_hash(id), n_shards); }

uint64_t nfagg_ip_hash(const uint8_t ip[16], uint32_t seed_index) {
    uint64_t lo, hi;
    memcpy(&lo, ip, 8); memcpy(&hi, ip + 8, 8);
    return ip_hash(lo, hi, seed_index);
}

int nfagg_sync(nfagg_handle* h) {
    if (!h) return NFAGG_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NFAGG_OK;
}

void* nfagg_stream(nfagg_handle* h) { return h ? (void*)h->stream : nullptr; }

int nfagg_debug_skip_sequence(nfagg_handle* h, uint64_t records) {
    if (!h) return NFAGG_EINVAL;
    h->epoch_seq += records;                                    // any amount: the window follows (nfagg_rebase.hip)
    return NFAGG_OK;
}

uint64_t nfagg_debug_live_buffers(void) { return g_live_buffers.load(); }

int nfagg_stats_get(nfagg_handle* h, nfagg_stats* out) {
    if (!h || !out) return fail(h, NFAGG_EINVAL, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = refresh_counters(h);
    if (rc != NFAGG_OK) return rc;
    prof_resolve(h);
    h->stats.entries = h->live;
    h->stats.epoch_seq = h->epoch_seq;
    *out = h->stats;
    return NFAGG_OK;
}

#ifdef NFAGG_DIAG
extern "C" {
// libnfagg_diag.so only: what the last epochs-found-first launch of nfagg_account saw — its control words and its cuts (host copies)
int nfagg_debug_last_cuts(nfagg_handle* h, uint32_t ctl[8], uint32_t* cuts, size_t cap) {
    if (!h || !ctl || !h->h_par) return NFAGG_EINVAL;
    for (int k = 0; k < 8; k++) ctl[k] = h->h_par[k];
    for (size_t k = 0; k < cap && k < 65535; k++) cuts[k] = h->h_par[512 + k];
    return NFAGG_OK;
}
int nfagg_debug_last_analysis(nfagg_handle* h, uint64_t* keys_sorted, int32_t* prev, uint32_t* pos, size_t n) {
    if (!h || !h->par.keys_sorted) return NFAGG_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    if (keys_sorted) HIP_TRY(h, hipMemcpy(keys_sorted, h->par.keys_sorted.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (prev) HIP_TRY(h, hipMemcpy(prev, h->par.prev.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (pos) HIP_TRY(h, hipMemcpy(pos, h->par.pos.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return NFAGG_OK;
}
// libnfagg_diag.so only: the dense-identity timing experiment of k_finalize + k_evict (nfagg_kernels.hip g_diag_dense). on = 1: a
// buffer of one 64-byte unit per slot is allocated and every table of the PROCESS uses it (one table at a time); 0: back to the
// cold half lines. Evicted MACs are wrong while it is on.
int nfagg_debug_dense_identity(nfagg_handle* h, int on) {
    static void* buf = nullptr;
    if (!h) return NFAGG_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    if (buf) { (void)hipFree(buf); buf = nullptr; }
    if (on) HIP_TRY(h, hipMalloc(&buf, (size_t)h->slots * 64));
    HIP_TRY(h, diag_set_dense(buf));
    return NFAGG_OK;
}
// libnfagg_diag.so only (not part of the drop-in ABI): per-phase wave-cycle sums of the phase-timing builds (variants 6/8/9).
int nfagg_debug_phase_cycles(nfagg_handle* h, uint64_t out[8]) {
    if (!h || !out) return NFAGG_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = refresh_counters(h);
    if (rc != NFAGG_OK) return rc;
    for (int k = 0; k < 8; k++) out[k] = h->h_ctr->phase[k];
    return NFAGG_OK;
}
}  // extern "C"
#endif

int nfagg_stats_reset_profile(nfagg_handle* h) {
    if (!h) return NFAGG_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    prof_resolve(h);
    h->stats.ingest_launches = h->stats.evict_launches = h->stats.sketch_launches = 0;
    h->stats.ingest_kernel_ms = h->stats.evict_kernel_ms = h->stats.sketch_kernel_ms = 0.0;
    return NFAGG_OK;
}
