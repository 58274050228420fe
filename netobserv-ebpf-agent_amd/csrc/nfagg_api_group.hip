// nfagg_api_group.hip — the multi-GPU group: it drives the members through the handle's internals (nfagg_api_core.h).
// include/nfagg.h documents the entry points.
//
// The Go agent is ONE process (pkg/agent/agent.go:387-442 builds one pipeline around one Accounter, constructed at
// agent.go:208-212), so N GPUs are driven from one process: every member is an ordinary nfagg_handle owning the flows
// whose key hashes to its shard (nfagg_shard_of). A batch enters through one member's device ("source": the one whose
// PCIe link the chunk arrived on, or wherever the caller has it), is partitioned there by a STABLE device partition
// (nfagg_partition.hip) and the buckets travel to their owners over xGMI (hipMemcpyPeerAsync), each owner folds its
// bucket on its own stream. Flow state needs no collective. The sketches are merged at the tick: RCCL ncclAllReduce
// (sum of uint64 Count-Min counters, max of the one-byte HLL registers: ncclUint8) in place on every member — librccl is loaded on demand
// (dlopen), a single-GPU process never pays for it.
//
// Capacity: CACHE_MAX_FLOWS is divided evenly, each shard holds at most ceil(max_entries / N) flows. A record whose new
// key finds ITS shard full stops the group exactly there (NFAGG_FULL + consumed, as account.go:85-94 stops at the record
// that finds the map full), and the caller evicts the whole group — the reference evicts its whole map.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <stdarg.h>
#include <stdio.h>
#include <atomic>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "nfagg_api_core.h"

using namespace nfagg;

namespace {

struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

bool rccl_load(RcclApi& r, std::string& err) {
    if (r.lib) return true;
    r.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!r.lib) r.lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!r.lib) { err = std::string("cannot load librccl: ") + dlerror(); return false; }
    r.CommInitAll = (decltype(r.CommInitAll))dlsym(r.lib, "ncclCommInitAll");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
    r.AllReduce = (decltype(r.AllReduce))dlsym(r.lib, "ncclAllReduce");
    r.GroupStart = (decltype(r.GroupStart))dlsym(r.lib, "ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))dlsym(r.lib, "ncclGroupEnd");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.lib, "ncclGetErrorString");
    if (!r.CommInitAll || !r.CommDestroy || !r.AllReduce || !r.GroupStart || !r.GroupEnd || !r.GetErrorString) {
        err = "librccl lacks a required symbol"; return false;
    }
    return true;
}

__global__ void k_sum_u64(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] += src[i];
}
__global__ void k_max_u8(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = dst[i] > src[i] ? dst[i] : src[i];
}

}  // namespace

struct nfagg_group {
    uint32_t n = 0;
    std::vector<nfagg_handle*> m;
    std::vector<int> dev;
    bool distinct = true;             // every member on its own device: RCCL. All on ONE device (test rig): local kernels.
    RcclApi rccl;
    std::vector<ncclComm_t> comm;
    struct Dst { DevBuf bucket; Event arrived, folded; };     // bucket: on the OWNER's device (freed with that device current)
    struct Src {                      // member i as SOURCE of a routed chunk: partition scratch on its device, its own stream for the
                                      // partition and the peer copies (the member's fold stream is busy with the buckets it owns), and
                                      // per owner j the landing area on j's device + the events that order its reuse. Everything
                                      // here is touched by ONE host thread at a time (the one feeding member i), outside fold_mu.
        DevBuf out, orig, scratch;
        DevBuf count;                                      // [0..64) bucket sizes, [64..128) prefix counts
        PinnedBuf count_mirror;
        uint64_t* h_count = nullptr;                       // = count_mirror, 128 words
        Stream pstream;
        std::vector<Dst> to;                               // [owner]
    };
    std::vector<Src> src;
    std::mutex fold_mu;               // routed mode: the members' tables and counters (everything after the partition of a call)
    uint32_t rr = 0;                  // host ingest: source member of the next chunk (spreads the chunks over the PCIe links)
    std::atomic<bool> must_evict{false};
    std::atomic<uint64_t> records_ingested{0}, full_stops{0};
    // A failure after the tables have been changed by part of a multi-member operation (some members folded, some slots
    // merged into their owners, some shards evicted) cannot be retried: the repeated operation would count twice what the
    // first attempt already applied. The group then refuses everything but nfagg_group_destroy.
    std::atomic<bool> failed{false};
    // ---- local-fold mode (NFAGG_GROUP_LOCAL_FOLD, nfagg_combine.hip)
    bool local = false;
    std::atomic<uint64_t> seq{0};     // next sequence number of the epoch, global to the group (ranges are reserved per call:
                                      // distinct members may be fed from distinct host threads)
    uint64_t origin = 0;              // start of the members' common 32-bit sequence window (nfagg_rebase.hip)
    std::mutex seq_mu;                // reservations, and the consolidation that moves the window
    std::atomic<uint32_t> inflight{0};// member folds between their reservation and their return
    uint64_t consolidations = 0;
    bool merged = false;              // the members' slots have been merged into their owners; only the eviction may follow
    struct Raw {                      // member i's live flows as partials grouped by owner, on its own device, at the eviction
        DevBuf d;
        uint64_t counts[64] = {}, off[64] = {};
        uint64_t owned = 0;
    };
    std::vector<Raw> raw;
    std::vector<Dst> peer;            // [owner * n + source]: landing area on the owner's device for a source on another device
    std::mutex err_mu;
    std::string err;
};

namespace {

int gfail(nfagg_group* g, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (g) { std::lock_guard<std::mutex> lk(g->err_mu); g->err = buf; } else return fail(nullptr, code, "%s", buf);
    return code;
}
int group_refuse_failed(nfagg_group* g) {
    std::string why;
    { std::lock_guard<std::mutex> lk(g->err_mu); why = g->err; }     // ingest threads may be reporting at the same time
    if (why.compare(0, 9, "the group") == 0) return NFAGG_ESTATE;     // already the refusal text: keep the first cause readable
    return gfail(g, NFAGG_ESTATE, "the group failed part-way through a multi-member operation and cannot continue (destroy it): %s", why.c_str());
}
int member_fail(nfagg_group* g, uint32_t j, int rc) { return gfail(g, rc, "member %u: %s", j, g->m[j]->err.c_str()); }

#define G_TRY(g, expr)                                                                                           \
    do { hipError_t e_ = (expr);                                                                                 \
         if (e_ != hipSuccess) return gfail((g), NFAGG_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

// Grow-only scratch of the group on member j's device (current): the member reports, the group passes it on.
int g_ensure(nfagg_group* g, uint32_t j, DevBuf& b, size_t need) {
    const int rc = b.ensure(g->m[j], need);
    return rc == NFAGG_OK ? rc : member_fail(g, j, rc);
}

// Fold the first cnt[j] records of every member's bucket; all members optimistic when any of them might cross its share.
// *crossed / *aborted: some member found its shard full / refused claims; stop[j] = bucket-relative index of the record that
// found shard j full (valid when crossed and not aborted). When nothing crossed the fold is committed.
int group_fold(nfagg_group* g, nfagg_group::Src& S, const std::vector<const void*>& bucket, const std::vector<uint64_t>& cnt, bool might,
               bool* crossed, bool* aborted, std::vector<uint64_t>& stop, std::vector<char>& hit) {
    *crossed = false; *aborted = false;
    int rc;
    if (!might) {
        for (uint32_t j = 0; j < g->n; j++) {
            nfagg_handle* h = g->m[j];
            if (!cnt[j]) continue;
            G_TRY(g, hipSetDevice(g->dev[j]));
            if ((rc = launch_ingest_profiled(h, bucket[j], cnt[j], h->epoch_seq)) != NFAGG_OK) return member_fail(g, j, rc);
            h->live_ub += cnt[j]; h->epoch_seq += cnt[j]; h->stats.records_ingested += cnt[j];
            G_TRY(g, hipEventRecord(S.to[j].folded, h->stream));
        }
        return NFAGG_OK;
    }
    std::vector<OptState> st(g->n);
    for (uint32_t j = 0; j < g->n; j++) {          // counters are fresh: the caller refreshed them to decide `might`
        G_TRY(g, hipSetDevice(g->dev[j]));
        if ((rc = opt_begin(g->m[j], st[j])) != NFAGG_OK) return member_fail(g, j, rc);
        if ((rc = opt_fold(g->m[j], st[j], bucket[j], cnt[j])) != NFAGG_OK) return member_fail(g, j, rc);
        G_TRY(g, hipEventRecord(S.to[j].folded, g->m[j]->stream));
    }
    for (uint32_t j = 0; j < g->n; j++) {
        G_TRY(g, hipSetDevice(g->dev[j]));
        bool c = false, a = false; uint64_t s = 0;
        if ((rc = opt_result(g->m[j], st[j], cnt[j], &c, &a, &s)) != NFAGG_OK) return member_fail(g, j, rc);
        hit[j] = c && !a; stop[j] = s;
        *crossed |= c; *aborted |= a;
    }
    for (uint32_t j = 0; j < g->n; j++) {
        G_TRY(g, hipSetDevice(g->dev[j]));
        if (!*crossed) opt_commit(g->m[j], st[j], cnt[j]);
        else if ((rc = opt_rollback(g->m[j], st[j])) != NFAGG_OK) return member_fail(g, j, rc);
    }
    return NFAGG_OK;
}

// Local-fold mode: the chunk is folded where it is, by member s, whatever its keys; sequence numbers continue the group's.
// The range [seq, seq + n) is reserved before the fold, so distinct members may be fed concurrently from distinct host
// threads (arrival order = order of the reservations); when the member stops early the rest of the range stays unused —
// only the order of sequence numbers matters.
int group_consolidate(nfagg_group* g);

int group_ingest_local(nfagg_group* g, uint32_t s, const void* d_records, size_t n, size_t* consumed_out) {
    nfagg_handle* h = g->m[s];
    size_t done = 0;
    int rc = NFAGG_OK;
    while (done < n && rc == NFAGG_OK) {
        const size_t m = (n - done) < (size_t)kMaxFoldChunk ? (n - done) : (size_t)kMaxFoldChunk;
        G_TRY(g, hipSetDevice(g->dev[s]));                       // before the reservation: nothing below may return with `inflight` raised
        uint64_t base;
        {   // reserve [base, base + m). An epoch has no maximum length: when the members' common 32-bit window is used up the
            // flows are brought together at their owners and the window moves (group_consolidate) — nobody is folding meanwhile.
            std::lock_guard<std::mutex> lk(g->seq_mu);
            if (g->seq.load() + m - g->origin >= kSeqWindow) {
                if (h->tv.subflow) {
                    // kernel-dedup mode: the window of sub-flow tables does not move (nfagg_config.local_fold): the epoch ends here
                    g->must_evict = true; g->full_stops++;
                    rc = NFAGG_FULL;
                    break;
                }
                while (g->inflight.load() != 0 && !g->failed.load()) std::this_thread::yield();
                if (g->failed.load()) { rc = group_refuse_failed(g); break; }
                if ((rc = group_consolidate(g)) != NFAGG_OK) break;
            }
            base = g->seq.fetch_add(m);
            g->inflight++;
        }
        h->epoch_seq = base;
        size_t c = 0;
        rc = ingest_device_core(h, (const char*)d_records + done * kRecordBytes, m, &c);
        g->inflight--;
        g->records_ingested += c;
        done += c;
        if (rc == NFAGG_FULL) { g->must_evict = true; g->full_stops++; }
        else if (rc != NFAGG_OK) rc = member_fail(g, s, rc);
        else if (c < m) break;
    }
    if (consumed_out) *consumed_out = done;
    return rc;
}

// Local-fold mode, first half of the eviction: every member exports its live flows as partials grouped by owner
// (nfagg_combine.hip; its own flows stay where they are), segment j of member i's export travels to owner j — over xGMI
// when the devices differ: 192 B per (flow, member) / N per link instead of the whole export — and j merges it. Runs once
// per epoch (g->merged): an eviction that comes back NFAGG_TRUNCATED is repeated with larger buffers from the merged state.
// Stage A (exports, landing areas) changes no table: a failure there (ENOMEM ...) leaves the eviction repeatable. From the
// first merge launch on a failure is final (g->failed): merging again would add the merged bytes and packets twice.
int group_local_merge(nfagg_group* g) {
    const uint32_t N = g->n;
    const size_t pbytes = nfagg_partial_bytes(g->m[0]);          // 192, or 256 for the sub-flow partials of the kernel-dedup mode
    int rc;
    for (uint32_t i = 0; i < N; i++) {
        nfagg_handle* h = g->m[i];
        nfagg_group::Raw& R = g->raw[i];
        G_TRY(g, hipSetDevice(g->dev[i]));
        for (uint32_t o = 0; o < 64; o++) { R.counts[o] = 0; R.off[o] = 0; }
        if (N == 1) continue;
        if ((rc = refresh_counters(h)) != NFAGG_OK) return member_fail(g, i, rc);
        if ((rc = g_ensure(g, i, R.d, (size_t)h->h_ctr->n_live * pbytes + 64)) != NFAGG_OK) return rc;
        size_t n_exp = 0;
        if ((rc = partials_export_core(h, N, i, R.d.p, (size_t)h->h_ctr->n_live, R.counts, &n_exp)) != NFAGG_OK) return member_fail(g, i, rc);
        uint64_t at = 0;
        for (uint32_t o = 0; o < N; o++) { R.off[o] = at; at += R.counts[o]; }
    }
    for (uint32_t j = 0; j < N; j++)                             // landing areas on the owners' devices
        for (uint32_t i = 0; i < N; i++) {
            if (i == j || g->dev[i] == g->dev[j] || !g->raw[i].counts[j]) continue;
            G_TRY(g, hipSetDevice(g->dev[j]));
            nfagg_group::Dst& P = g->peer[(size_t)j * N + i];
            if ((rc = g_ensure(g, j, P.bucket, (size_t)g->raw[i].counts[j] * pbytes + 64)) != NFAGG_OK) return rc;
        }
    // ---- stage B: the tables change from here on
    auto merge_all = [&]() -> int {
        for (uint32_t r = 1; r < N; r++) {                         // round r: owner j takes member j+r's segment (every link busy once per round)
            for (uint32_t j = 0; j < N; j++) {
                const uint32_t i = (j + r) % N;
                const nfagg_group::Raw& R = g->raw[i];
                const uint64_t cnt = R.counts[j];
                if (cnt == 0) continue;
                nfagg_handle* h = g->m[j];
                G_TRY(g, hipSetDevice(g->dev[j]));
                const char* at = R.d.as<const char>() + R.off[j] * pbytes;      // complete: the export synchronised
                if (g->dev[i] != g->dev[j]) {
                    nfagg_group::Dst& P = g->peer[(size_t)j * N + i];
                    G_TRY(g, hipMemcpyPeerAsync(P.bucket.p, g->dev[j], at, g->dev[i], (size_t)cnt * pbytes, h->stream));
                    at = P.bucket.as<const char>();
                }
                if ((rc = partials_merge_core(h, N, j, at, (size_t)cnt)) != NFAGG_OK) return member_fail(g, j, rc);
            }
        }
        for (uint32_t j = 0; j < N; j++) {
            if ((rc = owned_count_core(g->m[j], N, j, &g->raw[j].owned, nullptr)) != NFAGG_OK) return member_fail(g, j, rc);
            g->m[j]->exported = true;                              // also for N = 1: the member is evicted through evict_owned_core
        }
        return NFAGG_OK;
    };
    if ((rc = merge_all()) != NFAGG_OK) { g->failed = true; return rc; }
    // the other members' exports were read by kernels on the owners' streams: owned_count_core synchronised all of them
    g->merged = true;
    g->must_evict = true;            // a flow merged into its owner still sits in the other tables: nothing may be folded on top
    return NFAGG_OK;
}

// Moving the sequence window of a local-fold group (nfagg_rebase.hip, "across GPUs"): every member exports ALL its flows as
// partials grouped by owner, empties its table (epoch tag), every owner takes in the segments of the flows it owns — its own
// included — and rebases the single copy it now holds. No flow leaves the epoch: the next eviction delivers exactly what one
// Accounter over all the records would (tests/test_sequence_window_gpu.py). Called with seq_mu held and no fold in flight.
int group_consolidate(nfagg_group* g) {
    const uint32_t N = g->n;
    int rc;
    for (uint32_t i = 0; i < N; i++) {                             // stage A: exports and landing areas — no table changes
        nfagg_handle* h = g->m[i];
        nfagg_group::Raw& R = g->raw[i];
        G_TRY(g, hipSetDevice(g->dev[i]));
        if (h->must_evict) return gfail(g, NFAGG_ESTATE, "member %u has an eviction on full pending", i);
        if ((rc = refresh_counters(h)) != NFAGG_OK) return member_fail(g, i, rc);
        if ((rc = g_ensure(g, i, R.d, (size_t)h->h_ctr->n_live * kPartialBytes + 64)) != NFAGG_OK) return rc;
        size_t n_exp = 0;
        if ((rc = partials_export_core(h, N, NFAGG_SHARD_NONE, R.d.p, (size_t)h->h_ctr->n_live, R.counts, &n_exp)) != NFAGG_OK) return member_fail(g, i, rc);
        uint64_t at = 0;
        for (uint32_t o = 0; o < N; o++) { R.off[o] = at; at += R.counts[o]; }
    }
    for (uint32_t j = 0; j < N; j++)
        for (uint32_t i = 0; i < N; i++) {
            if (g->dev[i] == g->dev[j] || !g->raw[i].counts[j]) continue;
            G_TRY(g, hipSetDevice(g->dev[j]));
            nfagg_group::Dst& P = g->peer[(size_t)j * N + i];
            if ((rc = g_ensure(g, j, P.bucket, (size_t)g->raw[i].counts[j] * kPartialBytes + 64)) != NFAGG_OK) return rc;
        }
    const uint64_t next_seq = g->seq.load();
    auto restart = [&]() -> int {                                  // stage B: the tables change
        for (uint32_t j = 0; j < N; j++) if ((rc = window_clear_core(g->m[j])) != NFAGG_OK) return member_fail(g, j, rc);
        for (uint32_t r = 0; r < N; r++) {
            for (uint32_t j = 0; j < N; j++) {
                const uint32_t i = (j + r) % N;
                const nfagg_group::Raw& R = g->raw[i];
                const uint64_t cnt = R.counts[j];
                if (cnt == 0) continue;
                nfagg_handle* h = g->m[j];
                G_TRY(g, hipSetDevice(g->dev[j]));
                const char* at = R.d.as<const char>() + R.off[j] * kPartialBytes;
                if (g->dev[i] != g->dev[j]) {
                    nfagg_group::Dst& P = g->peer[(size_t)j * N + i];
                    G_TRY(g, hipMemcpyPeerAsync(P.bucket.p, g->dev[j], at, g->dev[i], (size_t)cnt * kPartialBytes, h->stream));
                    at = P.bucket.as<const char>();
                }
                if ((rc = partials_merge_core(h, N, j, at, (size_t)cnt)) != NFAGG_OK) return member_fail(g, j, rc);
            }
        }
        for (uint32_t j = 0; j < N; j++) if ((rc = window_finish_core(g->m[j], next_seq)) != NFAGG_OK) return member_fail(g, j, rc);
        return NFAGG_OK;
    };
    if ((rc = restart()) != NFAGG_OK) { g->failed = true; return rc; }
    g->origin = next_seq - rebase_keep();
    g->consolidations++;
    return NFAGG_OK;
}

// Local-fold mode, second half: member j writes the flows it owns to d_out (device memory of j, room for raw[j].owned records).
int group_local_evict_member(nfagg_group* g, uint32_t j, int reason, void* d_out) {
    nfagg_handle* h = g->m[j];
    G_TRY(g, hipSetDevice(g->dev[j]));
    size_t n = 0;
    const int rc = evict_owned_core(h, reason, g->n, j, d_out, (size_t)g->raw[j].owned, &n);
    if (rc != NFAGG_OK || n != (size_t)g->raw[j].owned) {
        g->failed = true;              // earlier members are in the next epoch already
        return rc != NFAGG_OK ? member_fail(g, j, rc) : gfail(g, NFAGG_EDEVICE, "member %u: evicted %zu flows, expected %llu", j, n, (unsigned long long)g->raw[j].owned);
    }
    return NFAGG_OK;
}

void group_local_epoch_done(nfagg_group* g) { g->seq = 0; g->origin = 0; g->merged = false; g->must_evict = false; }

// nothing folded since the last eviction anywhere (account.go:64-66: the timeout arm does not evict an empty map)
bool group_local_empty(nfagg_group* g) {
    if (g->merged || g->seq.load() != 0) return false;
    for (uint32_t j = 0; j < g->n; j++) if (g->m[j]->epoch_seq != 0 || g->m[j]->live_ub != 0) return false;
    return true;
}

// Routed mode. Two halves: the PARTITION of the chunk on the source's device (its own stream, its own buffers: one host thread
// per source member may be inside it at a time, concurrently with the others — round 2 ran it on the source member's fold stream
// and blocked the caller on it, so eight members' 8 ms partitions ran one after another), then, under fold_mu, the FOLD of the
// buckets by their owners (the members' tables, counters and sequence numbers: arrival order = the order in which calls take
// the lock).
int group_ingest_device_core(nfagg_group* g, uint32_t s, const void* d_records, size_t n, size_t* consumed_out) {
    if (consumed_out) *consumed_out = 0;
    if (g->failed) return group_refuse_failed(g);
    if (g->must_evict) return n ? NFAGG_FULL : NFAGG_OK;
    if (n == 0) return NFAGG_OK;
    if (g->local) return group_ingest_local(g, s, d_records, n, consumed_out);
    if (n >= (1ull << 31)) return gfail(g, NFAGG_ERANGE, "at most 2^31-1 records per group call");
    const uint32_t N = g->n;
    nfagg_group::Src& S = g->src[s];
    int rc;
    // ---- partition on the source device (buffers are reused: wait until the previous call's consumers are done)
    G_TRY(g, hipSetDevice(g->dev[s]));
    for (uint32_t j = 0; j < N; j++) G_TRY(g, hipStreamWaitEvent(S.pstream, S.to[j].folded, 0));
    if ((rc = g_ensure(g, s, S.out, n * kRecordBytes)) != NFAGG_OK) return rc;
    if ((rc = g_ensure(g, s, S.orig, n * sizeof(uint32_t))) != NFAGG_OK) return rc;
    if ((rc = g_ensure(g, s, S.scratch, partition_scratch_bytes(n, N))) != NFAGG_OK) return rc;
    if ((rc = g_ensure(g, s, S.count, 128 * sizeof(uint64_t))) != NFAGG_OK) return rc;
    uint64_t* d_count = S.count.as<uint64_t>();
    hipError_t e = launch_partition(d_records, n, N, S.out.p, S.orig.as<uint32_t>(), d_count, S.scratch.p, S.pstream);
    if (e != hipSuccess) return gfail(g, NFAGG_EDEVICE, "partition launch failed: %s", hipGetErrorString(e));
    G_TRY(g, hipMemcpyAsync(S.h_count, d_count, N * sizeof(uint64_t), hipMemcpyDeviceToHost, S.pstream));
    G_TRY(g, hipStreamSynchronize(S.pstream));                 // the partition of THIS chunk only: nobody's folds are waited for
    std::vector<uint64_t> cnt(N), off(N);
    uint64_t total = 0;
    for (uint32_t j = 0; j < N; j++) { cnt[j] = S.h_count[j]; off[j] = total; total += cnt[j]; }
    if (total != n) return gfail(g, NFAGG_EDEVICE, "partition lost records: %llu of %zu", (unsigned long long)total, n);
    // ---- the buckets travel to their owners (same device: folded where they lie), each into this source's landing area there
    std::vector<const void*> bucket(N);
    std::vector<char> remote(N, 0);
    for (uint32_t j = 0; j < N; j++) {
        const char* at = S.out.as<const char>() + off[j] * kRecordBytes;
        if (g->dev[j] == g->dev[s]) { bucket[j] = at; continue; }
        if (cnt[j]) {
            G_TRY(g, hipSetDevice(g->dev[j]));
            if ((rc = g_ensure(g, j, S.to[j].bucket, cnt[j] * kRecordBytes)) != NFAGG_OK) return rc;
            G_TRY(g, hipSetDevice(g->dev[s]));
            G_TRY(g, hipMemcpyPeerAsync(S.to[j].bucket.p, g->dev[j], at, g->dev[s], cnt[j] * kRecordBytes, S.pstream));
            G_TRY(g, hipEventRecord(S.to[j].arrived, S.pstream));
            remote[j] = 1;
        }
        bucket[j] = S.to[j].bucket.p;
    }
    // ---- from here on the members' tables: one call at a time
    std::lock_guard<std::mutex> fold_lock(g->fold_mu);
    if (g->failed) return group_refuse_failed(g);
    if (g->must_evict) return NFAGG_FULL;                      // another source's call found a shard full meanwhile: nothing of this chunk is folded
    for (uint32_t j = 0; j < N; j++) {                         // a member's bucket holds at most n < 2^31 records: room in its sequence window
        G_TRY(g, hipSetDevice(g->dev[j]));
        if ((rc = ensure_seq_window(g->m[j], n, nullptr)) != NFAGG_OK) return member_fail(g, j, rc);
        if (remote[j]) G_TRY(g, hipStreamWaitEvent(g->m[j]->stream, S.to[j].arrived, 0));
    }
    // ---- can any shard be filled by this call? (upper bounds first, exact counts only when needed)
    bool might = false;
    for (uint32_t j = 0; j < N; j++) might |= g->m[j]->live_ub + cnt[j] > g->m[j]->cfg.max_entries;
    if (might) {
        might = false;
        for (uint32_t j = 0; j < N; j++) {
            G_TRY(g, hipSetDevice(g->dev[j]));
            if ((rc = refresh_counters(g->m[j])) != NFAGG_OK) return member_fail(g, j, rc);
            might |= g->m[j]->live + cnt[j] > g->m[j]->cfg.max_entries;
        }
    }
    std::vector<uint64_t> stop(N, 0), part = cnt;
    std::vector<char> hit(N, 0);
    uint64_t prefix = n;                       // records of the call (in arrival order) being tried
    for (int attempt = 0; attempt < 64; attempt++) {
        bool crossed = false, aborted = false;
        // a member failing inside the fold leaves the earlier members folded (or half rolled back): not repeatable
        if ((rc = group_fold(g, S, bucket, part, might, &crossed, &aborted, stop, hit)) != NFAGG_OK) { g->failed = true; return rc; }
        if (!crossed) {
            g->records_ingested += prefix;
            if (consumed_out) *consumed_out = prefix;
            if (prefix < n) { g->must_evict = true; g->full_stops++; return NFAGG_FULL; }
            return NFAGG_OK;
        }
        // everything is rolled back. Where does the group stop? The earliest (in arrival order) record that found its shard
        // full; when claims were refused nobody knows: a quarter of the prefix next.
        uint64_t next = prefix / 4;
        if (!aborted) {
            next = prefix;
            G_TRY(g, hipSetDevice(g->dev[s]));
            for (uint32_t j = 0; j < N; j++) {
                if (!hit[j]) continue;
                uint32_t orig = 0;
                G_TRY(g, hipMemcpyAsync(&orig, S.orig.as<const uint32_t>() + off[j] + stop[j], sizeof orig, hipMemcpyDeviceToHost, S.pstream));
                G_TRY(g, hipStreamSynchronize(S.pstream));
                if (orig < next) next = orig;
            }
        }
        prefix = next;
        // bucket prefixes that make up records [0, prefix) of the call
        G_TRY(g, hipSetDevice(g->dev[s]));
        e = launch_partition_prefix_counts(S.orig.as<const uint32_t>(), d_count, N, prefix, d_count + 64, S.pstream);
        if (e != hipSuccess) return gfail(g, NFAGG_EDEVICE, "prefix count launch failed: %s", hipGetErrorString(e));
        G_TRY(g, hipMemcpyAsync(S.h_count + 64, d_count + 64, N * sizeof(uint64_t), hipMemcpyDeviceToHost, S.pstream));
        G_TRY(g, hipStreamSynchronize(S.pstream));
        for (uint32_t j = 0; j < N; j++) part[j] = S.h_count[64 + j];
        if (!aborted) might = false;           // exact stop: the prefixes fit by construction, fold them for good
        if (prefix == 0) {
            if (aborted) return gfail(g, NFAGG_EDEVICE, "group fold aborted on an empty prefix");
            g->must_evict = true; g->full_stops++;
            return NFAGG_FULL;
        }
    }
    return gfail(g, NFAGG_EDEVICE, "group fold did not converge");
}

}  // namespace

extern "C" {

int nfagg_group_create(const nfagg_config* cfg_in, const int32_t* devices, uint32_t n_devices, nfagg_group** out) {
    if (!cfg_in || !devices || !out || n_devices == 0) return gfail(nullptr, NFAGG_EINVAL, "null argument");
    if (n_devices > 64) return gfail(nullptr, NFAGG_EINVAL, "at most 64 members");
    if (cfg_in->struct_size != sizeof(nfagg_config)) return gfail(nullptr, NFAGG_EINVAL, "nfagg_config.struct_size mismatch");
    *out = nullptr;
    nfagg_group* g = new (std::nothrow) nfagg_group();
    if (!g) return gfail(nullptr, NFAGG_ENOMEM, "out of host memory");
    std::set<int> seen(devices, devices + n_devices);
    g->distinct = seen.size() == n_devices;
    if (!g->distinct && seen.size() != 1) {
        delete g;
        return gfail(nullptr, NFAGG_EINVAL, "members must be on distinct devices (or all on one device: single-GPU test rig)");
    }
    g->n = n_devices;
    g->src.resize(n_devices);
    g->local = (cfg_in->group_flags & NFAGG_GROUP_LOCAL_FOLD) != 0;
    if (cfg_in->group_flags & ~(uint32_t)NFAGG_GROUP_LOCAL_FOLD) { delete g; return gfail(nullptr, NFAGG_EINVAL, "unknown group_flags"); }
    if (g->local) { g->raw.resize(n_devices); g->peer.resize((size_t)n_devices * n_devices); }
    const uint64_t total = cfg_in->max_entries ? cfg_in->max_entries : 5000;
    for (uint32_t j = 0; j < n_devices; j++) {
        nfagg_config c = *cfg_in;
        c.device = devices[j];
        c.group_flags = 0; c.local_fold = 0;
        c.n_shards = n_devices; c.shard_id = j;
        c.max_entries = (total + n_devices - 1) / n_devices;          // CACHE_MAX_FLOWS divided evenly over the shards
        if (g->local) {
            // every member folds any key, so CACHE_MAX_FLOWS bounds each member's table undivided; at the eviction the table
            // also takes the flows it owns from the other members (about 1/N of the distinct flows): four slots per entry
            c.n_shards = 1; c.shard_id = 0; c.max_entries = total;
            c.local_fold = 1;                                         // kernel-dedup mode: members keyed by (flow, interface), joined at the eviction
            if (!c.table_log2_slots) { uint32_t b = 16; while ((1ull << b) < 4 * total) b++; c.table_log2_slots = b; }
            else if (c.table_log2_slots < 63 && (1ull << c.table_log2_slots) < 4 * total) {
                // the claim limit (3/4 of the slots) must cover max_entries of the member's own flows plus the flows it owns
                // from every other member: with fewer than 4 slots per entry the merge can run into it and the epoch is lost
                nfagg_group_destroy(g);
                return gfail(nullptr, NFAGG_EINVAL, "NFAGG_GROUP_LOCAL_FOLD needs table_log2_slots with 2^k >= 4 * max_entries (or 0 for the default)");
            }
        }
        for (int k = 0; k < 4; k++) c.ext_sketch[k] = nullptr;        // every member owns its sketches
        nfagg_handle* h = nullptr;
        int rc = nfagg_create(&c, &h);
        if (rc != NFAGG_OK) { nfagg_group_destroy(g); return rc; }    // g_create_error holds the reason
        h->ext_sequenced = g->local;                                  // local fold: one numbering for all members, windows move together
        g->m.push_back(h); g->dev.push_back(devices[j]);
        hipSetDevice(devices[j]);
        nfagg_group::Src& S = g->src[j];
        S.to.resize(n_devices);
        bool ok = S.pstream.create() == hipSuccess && S.count_mirror.alloc(128 * sizeof(uint64_t)) == hipSuccess;
        S.h_count = S.count_mirror.as<uint64_t>();
        // an event belongs to the device that is current when it is created and can only be recorded on a stream of that device
        // (any stream may WAIT for it): `arrived` is recorded on this source's stream, `folded` on owner k's fold stream
        for (uint32_t k = 0; ok && k < n_devices; k++) {
            ok = hipSetDevice(devices[j]) == hipSuccess && S.to[k].arrived.create() == hipSuccess &&
                 hipSetDevice(devices[k]) == hipSuccess && S.to[k].folded.create() == hipSuccess;
        }
        hipSetDevice(devices[j]);
        if (!ok) {
            nfagg_group_destroy(g);
            return gfail(nullptr, NFAGG_EDEVICE, "stream / event / pinned allocation failed");
        }
    }
    if (g->distinct) {
        for (uint32_t i = 0; i < n_devices; i++) {                     // direct peer access where the topology offers it
            hipSetDevice(devices[i]);
            for (uint32_t j = 0; j < n_devices; j++) {
                int can = 0;
                if (i != j && hipDeviceCanAccessPeer(&can, devices[i], devices[j]) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(devices[j], 0);
            }
        }
        (void)hipGetLastError();
        if (cfg_in->sketch_flags & (NFAGG_SKETCH_CM | NFAGG_SKETCH_HLL)) {
            std::string why;
            if (!rccl_load(g->rccl, why)) { nfagg_group_destroy(g); return gfail(nullptr, NFAGG_EDEVICE, "%s", why.c_str()); }
            g->comm.resize(n_devices);
            std::vector<int> devs(devices, devices + n_devices);
            const ncclResult_t r = g->rccl.CommInitAll(g->comm.data(), (int)n_devices, devs.data());
            if (r != ncclSuccess) {
                g->comm.clear();
                const std::string msg = g->rccl.GetErrorString(r);
                nfagg_group_destroy(g);
                return gfail(nullptr, NFAGG_EDEVICE, "ncclCommInitAll failed: %s", msg.c_str());
            }
        }
    }
    *out = g;
    return NFAGG_OK;
}

void nfagg_group_destroy(nfagg_group* g) {
    if (!g) return;
    for (uint32_t j = 0; j < g->m.size(); j++) { hipSetDevice(g->dev[j]); hipStreamSynchronize(g->m[j]->stream); }
    for (auto c : g->comm) if (c) g->rccl.CommDestroy(c);
    for (auto& S : g->src) if (S.pstream) hipStreamSynchronize(S.pstream);
    // the landing areas lie on their OWNERS' devices: each is freed with its own device current; everything else goes with the group
    for (auto& S : g->src)
        for (uint32_t k = 0; k < S.to.size() && k < g->dev.size(); k++) { hipSetDevice(g->dev[k]); S.to[k].bucket.reset(); }
    for (size_t q = 0; q < g->peer.size() && q / g->n < g->dev.size(); q++) { hipSetDevice(g->dev[q / g->n]); g->peer[q].bucket.reset(); }
    for (auto h : g->m) nfagg_destroy(h);
    delete g;
}

const char* nfagg_group_last_error(const nfagg_group* g) { return g ? g->err.c_str() : nfagg_last_error(nullptr); }

uint32_t nfagg_group_size(const nfagg_group* g) { return g ? g->n : 0; }

nfagg_handle* nfagg_group_member(nfagg_group* g, uint32_t i) { return (g && i < g->n) ? g->m[i] : nullptr; }

int nfagg_group_ingest_device(nfagg_group* g, uint32_t src_member, const void* d_records, size_t n, size_t* consumed) {
    if (!g || (!d_records && n) || src_member >= g->n) return gfail(g, NFAGG_EINVAL, "bad argument");
    if (((uintptr_t)d_records & 15u) != 0) return gfail(g, NFAGG_EINVAL, "device records must be 16-byte aligned");
    return group_ingest_device_core(g, src_member, d_records, n, consumed);
}

int nfagg_group_ingest(nfagg_group* g, const void* records, size_t n, size_t* consumed_out) {
    if (!g || (!records && n)) return gfail(g, NFAGG_EINVAL, "null argument");
    if (g->failed) return group_refuse_failed(g);
    size_t consumed = 0;
    int rc = NFAGG_OK;
    const char* srcp = static_cast<const char*>(records);
    while (consumed < n) {
        const uint32_t s = g->rr;                           // this chunk goes up the PCIe link of member s
        nfagg_handle* h = g->m[s];
        G_TRY(g, hipSetDevice(g->dev[s]));
        if ((rc = staging_alloc(h)) != NFAGG_OK) return member_fail(g, s, rc);
        const size_t cap = (size_t)h->cfg.staging_records;
        const size_t mrec = g->local ? stage_chunk(h, n - consumed, cap) : ((n - consumed) < cap ? (n - consumed) : cap);
        const int b = h->stage_next;
        G_TRY(g, hipEventSynchronize(h->stage_free[b]));
        staged_copy(h->pinned[b].p, srcp + consumed * kRecordBytes, mrec * kRecordBytes, h->cfg.copy_threads);
        G_TRY(g, hipMemcpyAsync(h->d_stage[b].p, h->pinned[b].p, mrec * kRecordBytes, hipMemcpyHostToDevice, h->copy_stream));
        G_TRY(g, hipEventRecord(h->stage_up[b], h->copy_stream));
        G_TRY(g, hipStreamWaitEvent(h->stream, h->stage_up[b], 0));
        if (!g->local) G_TRY(g, hipStreamWaitEvent(g->src[s].pstream, h->stage_up[b], 0));   // routed: the partition reads the chunk on the source's own stream
        size_t c = 0;
        rc = group_ingest_device_core(g, s, h->d_stage[b].p, mrec, &c);
        G_TRY(g, hipSetDevice(g->dev[s]));
        G_TRY(g, hipEventRecord(h->stage_free[b], h->stream));
        h->stage_next ^= 1;
        g->rr = (g->rr + 1) % g->n;
        consumed += c;
        if (rc != NFAGG_OK) break;
    }
    if (consumed_out) *consumed_out = consumed;
    return rc;
}

int nfagg_group_debug_skip_sequence(nfagg_group* g, uint64_t records) {
    if (!g) return NFAGG_EINVAL;
    std::lock_guard<std::mutex> lk(g->seq_mu);
    if (g->local) g->seq += records;
    else for (uint32_t j = 0; j < g->n; j++) g->m[j]->epoch_seq += records;
    return NFAGG_OK;
}

int nfagg_group_len(nfagg_group* g, uint64_t* entries) {
    if (!g || !entries) return gfail(g, NFAGG_EINVAL, "null argument");
    uint64_t total = 0;
    for (uint32_t j = 0; j < g->n; j++) {
        uint64_t v = 0;
        const int rc = nfagg_len(g->m[j], &v);
        if (rc != NFAGG_OK) return member_fail(g, j, rc);
        total += v;
    }
    *entries = total;
    return NFAGG_OK;
}

int nfagg_group_merge_sketches(nfagg_group* g) {
    if (!g) return NFAGG_EINVAL;
    if (g->failed) return group_refuse_failed(g);
    const uint32_t flags = g->m[0]->sk.flags;
    if (!flags || g->n == 1) return NFAGG_OK;
    const size_t cm_n = (flags & NFAGG_SKETCH_CM) ? ((size_t)g->m[0]->sk.cm_depth << g->m[0]->sk.cm_log2w) : 0;
    const size_t hll_n = (flags & NFAGG_SKETCH_HLL) ? ((size_t)1 << g->m[0]->sk.hll_p) : 0;
    if (g->distinct) {
        // RCCL all-reduce over xGMI, in place on every member, on the members' own streams (ordered after their folds)
        ncclResult_t r = g->rccl.GroupStart();
        for (uint32_t j = 0; j < g->n && r == ncclSuccess; j++) {
            nfagg_handle* h = g->m[j];
            for (int k = 0; k < 2 && r == ncclSuccess; k++) {
                if (cm_n) r = g->rccl.AllReduce(h->sk.cm[k], h->sk.cm[k], cm_n, ncclUint64, ncclSum, g->comm[j], h->stream);
                if (hll_n && r == ncclSuccess) r = g->rccl.AllReduce(h->sk.hll[k], h->sk.hll[k], hll_n, ncclUint8, ncclMax, g->comm[j], h->stream);   // 16 KiB at p = 14
            }
        }
        const ncclResult_t r2 = g->rccl.GroupEnd();
        if (r == ncclSuccess) r = r2;
        if (r != ncclSuccess) return gfail(g, NFAGG_EDEVICE, "ncclAllReduce failed: %s", g->rccl.GetErrorString(r));
        return NFAGG_OK;
    }
    // single-GPU test rig (all members on one device): same result with local kernels
    G_TRY(g, hipSetDevice(g->dev[0]));
    for (uint32_t j = 0; j < g->n; j++) G_TRY(g, hipStreamSynchronize(g->m[j]->stream));
    hipStream_t s0 = g->m[0]->stream;
    for (int k = 0; k < 2; k++) {
        for (uint32_t j = 1; j < g->n; j++) {
            (void)hipGetLastError();
            if (cm_n) hipLaunchKernelGGL(k_sum_u64, dim3(1024), dim3(256), 0, s0, g->m[0]->sk.cm[k], g->m[j]->sk.cm[k], cm_n);
            if (hll_n) hipLaunchKernelGGL(k_max_u8, dim3(64), dim3(256), 0, s0, g->m[0]->sk.hll[k], g->m[j]->sk.hll[k], hll_n);
            G_TRY(g, hipGetLastError());
        }
        for (uint32_t j = 1; j < g->n; j++) {
            if (cm_n) G_TRY(g, hipMemcpyAsync(g->m[j]->sk.cm[k], g->m[0]->sk.cm[k], cm_n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s0));
            if (hll_n) G_TRY(g, hipMemcpyAsync(g->m[j]->sk.hll[k], g->m[0]->sk.hll[k], hll_n, hipMemcpyDeviceToDevice, s0));
        }
    }
    G_TRY(g, hipStreamSynchronize(s0));
    return NFAGG_OK;
}

int nfagg_group_evict(nfagg_group* g, int reason, void* out, size_t cap, size_t* n_out) {
    if (!g || !n_out || reason < 0 || reason > 2) return gfail(g, NFAGG_EINVAL, "bad argument");
    if (g->failed) return group_refuse_failed(g);
    if (g->local) {
        int rc;
        *n_out = 0;
        if (reason == NFAGG_REASON_TIMEOUT && group_local_empty(g)) return NFAGG_OK;
        if (!g->merged && (rc = group_local_merge(g)) != NFAGG_OK) return rc;
        size_t total_owned = 0;
        for (uint32_t j = 0; j < g->n; j++) total_owned += (size_t)g->raw[j].owned;
        *n_out = total_owned;
        if (total_owned > cap) return NFAGG_TRUNCATED;
        if (total_owned && !out) return gfail(g, NFAGG_EINVAL, "null output buffer");
        size_t at = 0;
        for (uint32_t j = 0; j < g->n; j++) {
            nfagg_handle* h = g->m[j];
            const size_t nj = (size_t)g->raw[j].owned;
            G_TRY(g, hipSetDevice(g->dev[j]));
            if ((rc = h->d_evict.ensure(h, nj * kRecordBytes + 16)) != NFAGG_OK) return member_fail(g, j, rc);
            if ((rc = group_local_evict_member(g, j, reason, h->d_evict.p)) != NFAGG_OK) return rc;
            if (nj) G_TRY(g, hipMemcpy((char*)out + at * kRecordBytes, h->d_evict.p, nj * kRecordBytes, hipMemcpyDeviceToHost));
            at += nj;
        }
        group_local_epoch_done(g);
        return NFAGG_OK;
    }
    uint64_t total = 0;
    int rc = nfagg_group_len(g, &total);
    if (rc != NFAGG_OK) return rc;
    *n_out = (size_t)total;
    if (total > cap) return NFAGG_TRUNCATED;
    size_t at = 0;
    for (uint32_t j = 0; j < g->n; j++) {
        size_t nj = 0;
        rc = nfagg_evict(g->m[j], reason, (char*)out + at * kRecordBytes, cap - at, &nj);
        if (rc != NFAGG_OK) { if (j) g->failed = true; return member_fail(g, j, rc); }     // earlier shards are in the next epoch already
        at += nj;
    }
    *n_out = at;
    g->must_evict = false;
    return NFAGG_OK;
}

int nfagg_group_evict_device(nfagg_group* g, int reason, void* const* d_out, const size_t* cap, size_t* n_out) {
    if (!g || !d_out || !cap || !n_out || reason < 0 || reason > 2) return gfail(g, NFAGG_EINVAL, "bad argument");
    if (g->failed) return group_refuse_failed(g);
    if (g->local) {
        int rc;
        for (uint32_t j = 0; j < g->n; j++) n_out[j] = 0;
        if (reason == NFAGG_REASON_TIMEOUT && group_local_empty(g)) return NFAGG_OK;
        if (!g->merged && (rc = group_local_merge(g)) != NFAGG_OK) return rc;
        bool fits = true;
        for (uint32_t j = 0; j < g->n; j++) {
            n_out[j] = (size_t)g->raw[j].owned;
            fits &= n_out[j] <= cap[j];
            if (n_out[j] && (!d_out[j] || ((uintptr_t)d_out[j] & 15u))) return gfail(g, NFAGG_EINVAL, "device output %u null or not 16-byte aligned", j);
        }
        if (!fits) return NFAGG_TRUNCATED;
        for (uint32_t j = 0; j < g->n; j++)
            if ((rc = group_local_evict_member(g, j, reason, d_out[j])) != NFAGG_OK) return rc;
        group_local_epoch_done(g);
        return NFAGG_OK;
    }
    int worst = NFAGG_OK;
    for (uint32_t j = 0; j < g->n; j++) {       // sizes first: nothing is evicted unless every member's buffer is large enough
        uint64_t v = 0;
        const int rc = nfagg_len(g->m[j], &v);
        if (rc != NFAGG_OK) return member_fail(g, j, rc);
        n_out[j] = (size_t)v;
        if (v > cap[j]) worst = NFAGG_TRUNCATED;
    }
    if (worst != NFAGG_OK) return worst;
    for (uint32_t j = 0; j < g->n; j++) {
        const int rc = nfagg_evict_device(g->m[j], reason, d_out[j], cap[j], &n_out[j]);
        if (rc != NFAGG_OK) { if (j) g->failed = true; return member_fail(g, j, rc); }     // earlier shards are in the next epoch already
    }
    g->must_evict = false;
    return NFAGG_OK;
}

}  // extern "C"
