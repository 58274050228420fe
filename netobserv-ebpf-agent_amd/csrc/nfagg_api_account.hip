// nfagg_api_account.hip — nfagg_account / nfagg_account_device: the record arm of Accounter.Account WITH its evictions on "full"
// (include/nfagg.h), around the handle's fold and eviction (nfagg_api_core.h). Three ways through a call, tried in this order by
// account_device_core: the epochs found first (below), the kernel chain (account_chain_launch), the plain fold + eviction.
//
// The epochs found first: the host side of the evict-on-full loop with its epochs found first (kernels and
// the idea: nfagg_epoch_par.hip). THE path of nfagg_account[_device] for calls of more than a few epochs on an
// accounter-mode handle with max_entries <= kAccountParMaxEntries (the reference ships CACHE_MAX_FLOWS = 5000,
// pkg/config/config.go:146, deploys 10 000, scripts/agent.yml:35-36, and benchmarks 1 k / 10 k / 100 k,
// pkg/flow/tracer_map_bench_test.go:64-111); shorter calls, and calls this path declines, take the kernel chain
// (nfagg_epoch_chain.hip; up to kAccountFastMaxEntries) or the optimistic fold of nfagg_ingest (beyond).
//
// One launch handles up to 2^24 records of the call:
//   analysis   sort keys, sort, previous-occurrence links, live flags (main stream)
//   cut walk   in up to kParWalkParts parts, all enqueued at once (main stream, an event behind each; a part writes its cuts into the host's pinned list itself: the walk never waits for the host)
//   middle     every complete epoch, on a second stream, behind the part of the walk that completed it: positions, segment folds into the caller's buffer
//   epoch 0    records [0, cut 0): the ordinary fold into the table (it continues what the table holds), the ordinary eviction
//   tail       records from the last cut on: the ordinary fold (the epoch stays live) — only when the walk saw the call's end
// Same contract as account_chain_launch: *consumed records taken, *n_ep evictions of max_entries flows each appended to d_out
// (epoch_end[] relative to this launch's d_out), *stop = 2 when the room in d_out / epoch_end ended the launch early.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef NFAGG_DIAG
#include <chrono>
#endif
#include <thread>

#include "nfagg_api_core.h"

using namespace nfagg;

// ---------------------------------------------------------------- nfagg_account*: the record arm WITH its evictions on "full"
constexpr uint64_t kAccountFastMaxEntries = 32768;   // beyond that an epoch is long enough for the optimistic fold of nfagg_ingest

// May the device-resident epoch loop (the kernel chain, nfagg_epoch_chain.hip) take this batch?
static bool account_fast_ok(const nfagg_handle* h, size_t n, size_t out_cap) {
    // (a handle that filters its input by shard takes the host-driven loop: the chain counts the records it skips per window, and a
    // window that ends on "full" is looked at again from the split on)
    return h->cfg.mode == NFAGG_MODE_ACCOUNTER && h->cfg.n_shards <= 1 && h->cfg.max_entries <= kAccountFastMaxEntries && !h->must_evict && !h->exported &&
           h->cfg.max_entries + chain_window() + 16 <= h->tv.claim_limit && out_cap >= h->cfg.max_entries &&
           h->epoch_seq - h->seq_origin + n < kSeqWindow - chain_window() && (h->tv.epoch_bits >> 48) < 0xFFFFull;
}

// One pass of the kernel chain (nfagg_epoch_chain.hip) over d[0..n). *consumed / *n_ep / *n_out: records consumed, evictions
// performed, records written to d_out (epoch e ends at epoch_end[e] records); *stop as the control block reports it.
// Windows are enqueued kChainWindows[k] at a time, the control block is read back after each batch of launches.
// Windows per launch of the chain. A window takes up to chain_window() records and ends early where an epoch ends, so a call of n
// records needs about n / chain_window() + its evictions + 1 of them; the kernels of windows beyond the call's end find `stop` set
// and return at once — but a launch of nothing still costs ~2 us, and a shim that drains a 50-slot channel
// (pkg/agent/agent.go:408, pkg/config/config.go:134) calls with 1 ... a few thousand records: round 5 replayed 24 windows = 96
// launches for every call, 230 us for ONE record (profiles/r06_account_small_calls.txt). Three graphs, the shortest that covers
// what is left is replayed.
constexpr int kChainWindows[3] = {2, 6, 24};
constexpr size_t kChainEndsInline = 32;                 // epoch ends that come back with the control block (more: a second copy)

static int account_chain_launch(nfagg_handle* h, const void* d, size_t n, void* d_out, size_t out_cap, uint64_t* epoch_end, size_t max_epochs,
                                size_t* consumed, size_t* n_ep, size_t* n_out, uint32_t* stop) {
    int rc;
    // len(entries), n_live: the host knows them after an eviction and after the last chain launch (counters_exact) — one round
    // trip less per call; otherwise asked for
    if (!h->counters_exact) {
        if ((rc = refresh_counters(h)) != NFAGG_OK) return rc;
        if (h->h_ctr->n_finalized != h->h_ctr->n_live) return fail(h, NFAGG_ESTATE, "account: unfinalized slots at the start of a batch");
    }
    const uint64_t n_live0 = h->live_ub;
    const uint32_t me = max_epochs > 0xFFFFu ? 0xFFFFu : (uint32_t)max_epochs;
    const size_t ctlb = (chain_ctl_bytes() + 63) & ~(size_t)63;
    ChainScratch& C = h->chain;
    if ((rc = C.ctl.ensure(h, ctlb)) != NFAGG_OK) return rc;
    if ((rc = C.ends.ensure(h, (size_t)(me + 1) * sizeof(uint64_t))) != NFAGG_OK) return rc;
    if ((rc = C.live.ensure(h, (size_t)(h->cfg.max_entries + chain_window() + 64) * sizeof(uint32_t))) != NFAGG_OK) return rc;
    if ((rc = C.host.ensure(h, ctlb + (size_t)(me + 1) * sizeof(uint64_t))) != NFAGG_OK) return rc;
    void* const h_ep = C.host.p;
    const uint64_t seq_start = h->epoch_seq - h->seq_origin;                      // window-relative, as the slots carry it
    chain_ctl_fill(h_ep, d, d_out, n, seq_start, h->live, n_live0, out_cap, h->tv.epoch_bits, h->cfg.max_entries, me);
    HIP_TRY(h, hipMemcpyAsync(C.ctl.p, h_ep, chain_ctl_bytes(), hipMemcpyHostToDevice, h->stream));
    // kChainWindows[k] windows = 4 x that many launches whose arguments are the same in every call: captured into graphs once, one
    // hipGraphLaunch per batch afterwards (eager launches cost the host ~8 us each here: the chain was host-bound)
    if (!h->ep_graph_off && (!h->ep_graph[0] || h->ep_graph_key[0] != C.ctl.p || h->ep_graph_key[1] != C.ends.p || h->ep_graph_key[2] != C.live.p)) {
        hipError_t ec = hipSuccess;
        for (int k = 0; k < 3; k++) {
            h->ep_graph[k].reset();
            hipGraph_t g = nullptr;
            if (ec == hipSuccess) ec = hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal);
            else continue;
            if (ec == hipSuccess) {
                for (int w = 0; w < kChainWindows[k] && ec == hipSuccess; w++)
                    ec = launch_epoch_chain_window(h->tv, h->sk, C.ctl.p, C.live.as<uint32_t>(), C.ends.as<uint64_t>(), h->stream);
                const hipError_t ee = hipStreamEndCapture(h->stream, &g);
                if (ec == hipSuccess) ec = ee;
                if (ec == hipSuccess) ec = hipGraphInstantiate(&h->ep_graph[k].g, g, nullptr, nullptr, 0);
                if (g) hipGraphDestroy(g);
            }
        }
        if (ec != hipSuccess) {
            // no graph (a capture that something in the process invalidated, an instantiation that failed): this handle launches
            // its windows eagerly from now on — slower (~8 us of host time per launch), never wrong
            (void)hipGetLastError();
            for (int k = 0; k < 3; k++) h->ep_graph[k].reset();
            h->ep_graph_off = true;
        } else {
            h->ep_graph_key[0] = C.ctl.p; h->ep_graph_key[1] = C.ends.p; h->ep_graph_key[2] = C.live.p;
        }
    }
    EventPair ep{};
    if (h->cfg.profile) prof_begin(h, ep, 0);
    uint64_t v[9];
    uint64_t left = n, ends_inline = 0;
    h->counters_exact = false; h->mirror_fresh = false;
    for (;;) {
        // windows this launch should hold: what is left in whole windows, one for every eviction an epoch of max_entries flows can
        // end in (each ends its window early), one to spare
        const uint64_t want = (left + chain_window() - 1) / chain_window() + left / (h->cfg.max_entries ? h->cfg.max_entries : 1) + 1;
        int k = 0;
        while (k < 2 && (uint64_t)kChainWindows[k] < want) k++;
        if (h->ep_graph[k]) HIP_TRY(h, hipGraphLaunch(h->ep_graph[k], h->stream));
        else {
            for (int w = 0; w < kChainWindows[k]; w++) {
                const hipError_t el = launch_epoch_chain_window(h->tv, h->sk, C.ctl.p, C.live.as<uint32_t>(), C.ends.as<uint64_t>(), h->stream);
                if (el != hipSuccess) return fail(h, NFAGG_EDEVICE, "epoch chain launch failed: %s", hipGetErrorString(el));
            }
        }
        // the control block, the first epoch ends and the counters behind ONE wait (round 5: three)
        ends_inline = me < kChainEndsInline ? me : kChainEndsInline;
        HIP_TRY(h, hipMemcpyAsync(h_ep, C.ctl.p, chain_ctl_bytes(), hipMemcpyDeviceToHost, h->stream));
        if (ends_inline) HIP_TRY(h, hipMemcpyAsync((char*)h_ep + ctlb, C.ends.p, ends_inline * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        if ((rc = refresh_counters_enqueue(h)) != NFAGG_OK) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        chain_ctl_read(h_ep, v);
        if (v[6] != 0) break;
        left = n - v[0];
    }
    if (h->cfg.profile) prof_end(h, ep);
    const uint64_t pos = v[0], seq = v[1], live = v[2], out_pos = v[3], n_epochs = v[5];
    if (n_epochs > ends_inline) {
        HIP_TRY(h, hipMemcpyAsync((char*)h_ep + ctlb + ends_inline * sizeof(uint64_t), C.ends.as<const uint64_t>() + ends_inline,
                                  (size_t)(n_epochs - ends_inline) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if ((rc = refresh_counters_taken(h)) != NFAGG_OK) return rc;
    if (h->h_ctr->n_live != live)
        return fail(h, NFAGG_EDEVICE, "epoch chain: %llu claimed slots, len(entries) %llu", (unsigned long long)h->h_ctr->n_live, (unsigned long long)live);
    for (uint64_t k = 0; k < n_epochs && k < max_epochs; k++) epoch_end[k] = ((const uint64_t*)((const char*)h_ep + ctlb))[k];
    h->tv.epoch_bits = v[4];
    // identity dwords of the slots the epoch in progress claimed in this call, from the batch
    const bool began_here = v[8] != 0;
    const uint64_t first_rec = began_here ? v[7] : 0, seq_at_first = began_here ? 0 : seq_start;
    const hipError_t e = launch_finalize(h->tv, (const char*)d + first_rec * kRecordBytes, pos - first_rec, seq_at_first, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "finalize launch failed: %s", hipGetErrorString(e));
    if (n_epochs) h->seq_origin = 0;                            // an eviction inside the call restarted the epoch: a fresh window
    h->epoch_seq = h->seq_origin + seq; h->live = h->live_ub = live;
    h->counters_exact = true;
    h->mirror_fresh = false;                                    // (k_finalize moves n_finalized behind the mirror's back)
    h->epoch_unclustered = true;
    h->stats.records_ingested += pos;
    h->stats.evictions[NFAGG_REASON_FULL] += n_epochs;
    h->stats.evicted_flows[NFAGG_REASON_FULL] += out_pos;
    *consumed = (size_t)pos; *n_ep = (size_t)n_epochs; *n_out = (size_t)out_pos; *stop = (uint32_t)v[6];
    return NFAGG_OK;
}

#ifdef NFAGG_DIAG
static double diag_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define NF_DIAG_T(var) const double var = diag_now_ms()
#define NF_DIAG_PRINT(...) fprintf(stderr, __VA_ARGS__)
#else
#define NF_DIAG_T(var)
#define NF_DIAG_PRINT(...)
#endif

constexpr uint64_t kParMaxRecords = 1ull << 24;          // the sort key keeps the index in its low 24 bits (nfagg_epoch_par.hip kIdxBits)
constexpr uint32_t kParMaxCuts = 65535;
constexpr uint64_t kAccountParMaxEntries = 1ull << 22;   // (positions are 32 bits and epochs x max_entries <= the records of a launch: any size would do; beyond this the fold itself dominates)
constexpr int kParDeclined = 1000;                       // (internal) this call is not for this path: take the chain
constexpr uint64_t kParWalkPartsMax = 16;                // (events of the handle)
constexpr uint32_t kParStateAt = 512 + kParMaxCuts + 1;  // the parts' state words in the pinned list, behind the cuts
constexpr uint64_t kParWalkFewFrom = 7500;               // table sizes from which the walk runs in two parts
constexpr uint64_t kParWalkParts = 4;                    // the cut walk of a long launch runs in this many parts (the folds of one part overlap the walk of the next)

// How long a call must be for this path. Its cost hardly depends on the call's length up to ~128 Ki records (~0.3 ms: two dozen small
// launches and three round trips); the kernel chain costs ~60 us per WINDOW, and a window ends at 16 384 records or at an epoch's
// end, whichever comes first: a call of n records is about n / 16 384 + n / (an epoch's length) windows. With an epoch taken as
// 2 x max_entries records (2.8 x on the configs[1] stream; 1 x at least) the two meet at five windows:
//   n >= 5 / (1 / 16 384 + 1 / (2 max_entries))     — 31 k records at CACHE_MAX_FLOWS = 5000, 65 k at 32 768, never above 80 k —
// measured, libnfagg_diag.so with NFAGG_DIAG_PAR_MIN (profiles/r06x_par_entry_bar.txt): at 5000 entries a device-resident call
// of 32 Ki records takes 326 us on the chain and 294 here, one of 64 Ki 430 and 300. (Round 5's bar was 4 x max_entries + 65 536.)
// Beyond kAccountFastMaxEntries there is no chain: the alternative is nfagg_ingest's optimistic fold (fold, find the split, roll
// back, fold the prefix again — per eviction), and the same bar serves. Never below one chain window.
static uint64_t account_par_min_records(uint64_t M) {
#ifdef NFAGG_DIAG
    // A/B (libnfagg_diag.so only): NFAGG_DIAG_PAR_MIN = the entry bar in records, whatever the table's size
    static const uint64_t ov = getenv("NFAGG_DIAG_PAR_MIN") ? strtoull(getenv("NFAGG_DIAG_PAR_MIN"), nullptr, 10) : 0;
    if (ov) return ov;
#endif
    const uint64_t bar = 5ull * 16384ull * (2 * M) / (2 * M + 16384ull);
    return bar < 16384 ? 16384 : bar;
}

static bool account_par_ok(const nfagg_handle* h, size_t n, size_t out_cap) {
    const uint64_t M = h->cfg.max_entries;
    return h->cfg.ingest_variant != kVariantAccountChain && h->cfg.mode == NFAGG_MODE_ACCOUNTER && h->cfg.n_shards <= 1 && !h->tv.subflow &&
           M >= 1 && M <= kAccountParMaxEntries && !h->must_evict && !h->exported && !h->ext_sequenced && out_cap >= M &&
           n >= account_par_min_records(M) &&
           (M <= kAccountFastMaxEntries || !h->counters_exact || h->live + n > M) &&   // (a call that cannot fill the map needs no analysis: the plain fold takes it)
           (h->tv.epoch_bits >> 48) + 2 < 0xFFFFull;
}

// d[0..m) is known to create no more than the table has room for (the cut walk said so): folded without the "might it fill the
// table" machinery of ingest_device_core. live_after: len(entries) once it is folded.
static int par_fold_known(nfagg_handle* h, const void* d, uint64_t m, uint64_t live_after) {
    if (m == 0) return NFAGG_OK;
    int rc;
    bool blocked = false;
    if ((rc = ensure_seq_window(h, m, &blocked)) != NFAGG_OK) return rc;
    if (blocked) return fail(h, NFAGG_ESTATE, "account: the sequence window cannot move on this handle");   // (account_par_ok excludes such handles)
    if ((rc = launch_ingest_profiled(h, d, m, h->epoch_seq)) != NFAGG_OK) return rc;
    h->epoch_seq += m;
    h->live = h->live_ub = live_after;
    h->counters_exact = true;                                   // every new key of these records claims one slot: n_live == live
    h->stats.records_ingested += m;
    return NFAGG_OK;
}

static int account_par_launch(nfagg_handle* h, const void* d, size_t n, void* d_out, size_t out_cap, uint64_t* epoch_end, size_t max_epochs,
                              size_t* consumed, size_t* n_ep, size_t* n_out, uint32_t* stop) {
    int rc;
    *consumed = 0; *n_ep = 0; *n_out = 0; *stop = 0;
    const uint64_t M = h->cfg.max_entries;
    const uint64_t m = n < kParMaxRecords ? n : kParMaxRecords;
    if (!h->counters_exact && (rc = refresh_counters(h)) != NFAGG_OK) return rc;  // exact len(entries)
    const uint64_t live0 = h->live;
    // how many evictions this launch may perform: room in d_out, in epoch_end[], in the cut list
    uint64_t room_cuts = out_cap / M;
    if (room_cuts > max_epochs) room_cuts = max_epochs;
    uint64_t max_cuts = room_cuts;
    if (max_cuts > kParMaxCuts) max_cuts = kParMaxCuts;                          // (the list's size; the caller's loop comes back for more)
    if (max_cuts == 0) return kParDeclined;
    ParScratch& P = h->par;
    // (each on its own: a call that failed half way — pinned memory is scarce — leaves what it created, the next one completes it)
    if (!P.stream) HIP_TRY(h, P.stream.create());
    if (!P.done) HIP_TRY(h, P.done.create());
    if (!P.host) {
        if (P.host.alloc((kParStateAt + 4 * kParWalkPartsMax) * sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return fail(h, NFAGG_ENOMEM, "account: no pinned memory for the cut list"); }
        h->h_par = P.host.as<uint32_t>();
    }
    // ---- analysis
    if ((rc = P.keys.ensure(h, m * sizeof(uint64_t))) != NFAGG_OK) return rc;          // sort keys
    if ((rc = P.keys_sorted.ensure(h, m * sizeof(uint64_t))) != NFAGG_OK) return rc;          // sort keys, sorted
    if ((rc = P.prev.ensure(h, par_prev_entries(m) * sizeof(int32_t))) != NFAGG_OK) return rc;   // prev, padded for the walk's look-ahead
    if ((rc = P.pos.ensure(h, m * sizeof(uint32_t))) != NFAGG_OK) return rc;          // pos
    const uint64_t long_cap = m / par_seg_short() + 4096;                                           // long segments: disjoint unless flows share their hash bits; the kernel bounds the append
    if ((rc = P.long_segs.ensure(h, (long_cap + par_huge_cap()) * sizeof(uint32_t))) != NFAGG_OK) return rc;   // (+ the lists and chunk partials of the segments folded in chunks)
    if ((rc = P.rank_tiles.ensure(h, (par_rank_tiles(m) + 1) * sizeof(uint32_t))) != NFAGG_OK) return rc;   // heads per tile of the ranking
    if ((rc = P.ctl.ensure(h, (kParMaxCuts + 1 + 512) * sizeof(uint32_t))) != NFAGG_OK) return rc;      // [0] n_cuts [1] link overflow [2] bad [3] tail flows [4] n_long [5] n_huge [6] huge chunks; [512..) cuts
    size_t temp_bytes = 0;
    hipError_t e = launch_par_sort(nullptr, &temp_bytes, P.keys.as<const uint64_t>(), P.keys_sorted.as<uint64_t>(), m, h->stream);
    if (e != hipSuccess) return fail(h, NFAGG_EDEVICE, "sort size query failed: %s", hipGetErrorString(e));
    if ((rc = P.sort_tmp.ensure(h, temp_bytes + 16)) != NFAGG_OK) return rc;               // sort scratch
    uint32_t* ctl = P.ctl.as<uint32_t>();
    uint32_t* d_cuts = ctl + 512;
    const uint64_t* ks = P.keys_sorted.as<const uint64_t>();
    int32_t* prev = P.prev.as<int32_t>();
    NF_DIAG_T(t_0);
    EventPair pe{};
    bool pe_open = false;
    if (h->cfg.profile) { prof_begin(h, pe, 0); pe_open = true; }
    auto prof_close = [&]() { if (pe_open) { prof_end(h, pe); pe_open = false; } };
    auto prof_drop = [&]() { if (pe_open) { h->ev_free.push_back(pe); pe_open = false; } };    // an exit before the walk's end: the pair goes back, nothing is counted
    HIP_TRY(h, hipMemsetAsync(ctl, 0, 512 * sizeof(uint32_t), h->stream));
    HIP_TRY(h, hipMemsetD32Async((hipDeviceptr_t)(prev + m), par_prev_pad_value(), (size_t)(par_prev_entries(m) - m), h->stream));   // beyond the call: never new
    e = launch_par_hash(d, m, P.keys.as<uint64_t>(), h->stream);
    if (e == hipSuccess) e = launch_par_sort(P.sort_tmp.p, &temp_bytes, P.keys.as<const uint64_t>(), P.keys_sorted.as<uint64_t>(), m, h->stream);
    if (e == hipSuccess) e = launch_par_links(d, ks, m, prev, ctl + 1, h->stream);
    if (e == hipSuccess && live0) e = launch_par_live(h->tv, d, prev, m, h->stream);
    if (e != hipSuccess) { prof_drop(); return fail(h, NFAGG_EDEVICE, "epoch analysis launch failed: %s", hipGetErrorString(e)); }
    // ---- the cut walk, in parts, ALL of them enqueued now, an event behind each: a part leaves its cuts and its end state in the
    // host's pinned list itself (k_par_cuts), so the walk never waits for the host. The host waits for the events one by one and hands
    // the epochs each part completed to the segment folds on the second stream: epoch t (0 <= t < found - 1) = records
    // [cuts[t], cuts[t + 1]), max_entries flows each, to d_out[(1 + t) * max_entries ...). The walk holds one compute unit; the folds
    // of the epochs already cut use the rest while it goes on.
    const uint64_t n_blocks = par_walk_blocks(m);                                // (a multiple of four: the walk's loop takes four at a time)
    // How many parts: every part's folds cost ~0.14 ms whatever they hold (more with long epochs) + their share of ~0.8 ms per 8 M
    // records, and what follows the walk's end is the last part's folds. Short epochs make a long walk (a step per block and per cut)
    // that hides four parts' folds; from ~10 000 entries on the walk is short and two parts are best (8 M records, ms per call at
    // 1 / 2 / 3 / 4 / 6 parts: 5000 entries 3.10 2.76 2.68 2.64 2.65, 10 000: 2.76 2.56 2.71 2.77 3.24, 100 000: 2.67 2.66 2.83 2.97 3.43;
    // a shorter last part loses: profiles/r06x_walk_ungated.txt).
    uint64_t walk_parts = M < kParWalkFewFrom ? kParWalkParts : 2, last_pct = 100;
#ifdef NFAGG_DIAG
    if (const char* wp = getenv("NFAGG_DIAG_WALK_PARTS")) { walk_parts = strtoull(wp, nullptr, 10); if (walk_parts < 1) walk_parts = 1; if (walk_parts > kParWalkPartsMax) walk_parts = kParWalkPartsMax; }   // A/B (libnfagg_diag.so only): 1 = the walk as one launch
    if (const char* lp = getenv("NFAGG_DIAG_WALK_LAST")) { last_pct = strtoull(lp, nullptr, 10); if (last_pct < 1) last_pct = 1; if (last_pct > 100) last_pct = 100; }   // the last part's share of an equal part, per cent
#endif
    const uint64_t min_part = (256u << 10) / par_cut_span();                     // a part: at least 256 Ki records (a walk of less than 512 Ki: one part)
    uint64_t part_end[kParWalkPartsMax];
    uint32_t n_parts = 1;
    part_end[0] = n_blocks;
    if (n_blocks >= 2 * min_part && walk_parts > 1) {
        uint64_t W = walk_parts;
        if (n_blocks / W < min_part) W = n_blocks / min_part;                    // (>= 2)
        // W - 1 parts of x blocks and one of x * last_pct / 100: x = n_blocks / (W - 1 + last_pct / 100), in units of four blocks
        uint64_t x = (n_blocks * 100 + (W - 1) * 100 + last_pct - 1) / ((W - 1) * 100 + last_pct);
        x = (x + 3) & ~3ull;
        n_parts = 0;
        for (uint64_t b = x; b < n_blocks && n_parts + 1 < W; b += x) part_end[n_parts++] = b;
        part_end[n_parts++] = n_blocks;
    }
    uint32_t* const cuts = h->h_par + 512;                                       // written by the walk's parts (pinned, device-visible)
    uint32_t* const part_state = h->h_par + kParStateAt;                         // four words per part
    const char* base = static_cast<const char*>(d);
    char* obase = static_cast<char*>(d_out);
    uint32_t found = 0, t_done = 0;                                              // cuts known; middle epochs [0, t_done) handed to the folds
    bool mid_launched = false;
    // From the first fold launch on a failure must not leave the second stream running behind the caller's back (nor the parts of
    // the walk still queued: they write into the handle's buffers).
    auto join_middle = [&]() { prof_drop(); (void)hipStreamSynchronize(h->stream); if (mid_launched) (void)hipStreamSynchronize(P.stream); };
    for (uint32_t p = 0; p < n_parts; p++) {
        const uint64_t b_lo = p ? part_end[p - 1] : 0, b_hi = part_end[p];
        if (!P.part[p]) HIP_TRY_DO(h, P.part[p].create(), join_middle());
        part_state[4 * p] = 0xffffffffu;
        e = launch_par_cuts(prev, m, (uint32_t)M, (uint32_t)live0, d_cuts, (uint32_t)max_cuts, ctl, b_lo, b_hi, cuts, part_state + 4 * p, h->stream);
        if (b_hi == n_blocks) prof_close();
        if (e != hipSuccess) { join_middle(); return fail(h, NFAGG_EDEVICE, "cut walk launch failed: %s", hipGetErrorString(e)); }
        HIP_TRY_DO(h, hipEventRecord(P.part[p], h->stream), join_middle());
    }
    uint64_t tail_flows = 0;
    for (uint32_t p = 0; p < n_parts; p++) {
        HIP_TRY_DO(h, hipEventSynchronize(P.part[p]), join_middle());
        const uint32_t known = found;
        found = part_state[4 * p];
        tail_flows = part_state[4 * p + 1];
        if (part_state[4 * p + 2]) { join_middle(); return kParDeclined; }    // more flows sharing their hash bits than k_par_links looks through (set before any walk: nothing is folded yet)
        if (found > max_cuts || found < known || part_state[4 * p + 3] != known) { join_middle(); return fail(h, NFAGG_EDEVICE, "epoch analysis: %u cuts after %u, at most %llu asked for", found, known, (unsigned long long)max_cuts); }
        for (uint32_t k = known; k < found; k++)
            if (cuts[k] >= m || (k && cuts[k] <= cuts[k - 1])) { join_middle(); return fail(h, NFAGG_EDEVICE, "epoch analysis: cut %u at record %u of %llu", k, cuts[k], (unsigned long long)m); }
        if (found >= 2 && found - 1 > t_done) {
            e = launch_par_middle(d, ks, m, prev, d_cuts, t_done, found - 1, cuts[t_done], cuts[found - 1], (uint32_t)M, h->sk, P.pos.as<uint32_t>(),
                                  obase + M * kRecordBytes, P.long_segs.as<uint32_t>(), (uint32_t)long_cap, P.long_segs.as<uint32_t>() + long_cap, P.rank_tiles.as<uint32_t>(), ctl + 4, ctl + 2, P.stream);
            mid_launched = true;
            if (e != hipSuccess) { join_middle(); return fail(h, NFAGG_EDEVICE, "segment fold launch failed: %s", hipGetErrorString(e)); }
            t_done = found - 1;
        }
        if (found >= max_cuts) break;                                            // (the parts still queued find the list full and return)
    }
    h->h_par[0] = found; h->h_par[1] = 0; h->h_par[3] = (uint32_t)tail_flows;    // (nfagg_debug_par_cuts reads them here)
#ifdef NFAGG_DIAG
    HIP_TRY_DO(h, hipMemcpyAsync(h->h_par + 16, ctl + 16, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream), join_middle());
    HIP_TRY_DO(h, hipStreamSynchronize(h->stream), join_middle());
#endif
    NF_DIAG_T(t_1);
    for (int wv = 0; wv < 2; wv++)
        NF_DIAG_PRINT("[account par] cut walk, wave %d, Ki cycles: loads awaited %u, counted %u, to the barrier's end %u, totals %u, cut found + barrier %u, cut bookkeeping %u, loads issued %u\n",
                      wv ? 15 : 0, h->h_par[16 + 8 * wv], h->h_par[17 + 8 * wv], h->h_par[22 + 8 * wv], h->h_par[18 + 8 * wv], h->h_par[19 + 8 * wv], h->h_par[20 + 8 * wv], h->h_par[21 + 8 * wv]);
    const bool walked_to_the_end = found < max_cuts;                             // the walk stopped because the records ended, not the list
    if (found == 0) {                                                            // no eviction inside these records: they fit
        if ((rc = par_fold_known(h, d, m, live0 + tail_flows)) != NFAGG_OK) return rc;
        *consumed = (size_t)m;
        return NFAGG_OK;
    }
    const uint32_t n_mid = found - 1;
    if (mid_launched) HIP_TRY_DO(h, hipEventRecord(P.done, P.stream), join_middle());
    // ---- epoch 0: what the table holds, continued up to the first cut; then its eviction
    if ((rc = par_fold_known(h, d, cuts[0], M)) != NFAGG_OK) { join_middle(); return rc; }
    if (h->live != M) { join_middle(); return fail(h, NFAGG_EDEVICE, "account: %llu flows at the first cut, expected %llu", (unsigned long long)h->live, (unsigned long long)M); }
    size_t out_pos = 0, ep = 0;
    {
        size_t got = 0;
        rc = evict_core(h, NFAGG_REASON_FULL, obase, true, out_cap, &got);       // checks that exactly live (= max_entries) flows came out
        if (rc != NFAGG_OK) { join_middle(); return rc; }                        // (NFAGG_TRUNCATED cannot be: out_cap >= max_entries)
        out_pos = got;
        epoch_end[ep++] = out_pos;
    }
    NF_DIAG_T(t_2);
    // ---- the tail: the epoch that stays live — when the walk saw where these records end
    uint64_t taken = cuts[found - 1];
    if (walked_to_the_end) {
        if ((rc = par_fold_known(h, base + taken * kRecordBytes, m - taken, tail_flows)) != NFAGG_OK) { join_middle(); return rc; }
        taken = m;
    } else if (max_cuts == room_cuts) {
        *stop = 2;                                                               // the room for evictions ended the launch
    }
    // ---- join: the middle's evictions are in d_out; did every epoch hold max_entries flows?
    if (n_mid) {
        HIP_TRY_DO(h, hipStreamWaitEvent(h->stream, P.done, 0), join_middle());
        HIP_TRY(h, hipMemcpyAsync(h->h_par, ctl, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (h->h_par[2]) return fail(h, NFAGG_EDEVICE, "account: an epoch of the middle does not hold %llu flows (code %u)", (unsigned long long)M, h->h_par[2]);
        for (uint32_t t = 0; t < n_mid; t++) { out_pos += M; epoch_end[ep++] = out_pos; }
        h->stats.records_ingested += (uint64_t)cuts[found - 1] - cuts[0];
        h->stats.evictions[NFAGG_REASON_FULL] += n_mid;
        h->stats.evicted_flows[NFAGG_REASON_FULL] += (uint64_t)n_mid * M;
    }
    NF_DIAG_T(t_3);
    NF_DIAG_PRINT("[account par] %llu records, %u cuts: analysis %.2f ms, epoch 0 + eviction %.2f, tail + join %.2f\n", (unsigned long long)m, found, t_1 - t_0, t_2 - t_1, t_3 - t_2);
    *consumed = (size_t)taken; *n_ep = ep; *n_out = out_pos;
    return NFAGG_OK;
}


// d_out: DEVICE. epoch_end: HOST. Evictions append to d_out; *n_epochs of them, the e-th ends at record epoch_end[e].
static int account_device_core(nfagg_handle* h, const void* d_records, size_t n, void* d_out, size_t out_cap, uint64_t* epoch_end,
                               size_t max_epochs, size_t* n_epochs_out, size_t* consumed_out) {
    size_t consumed = 0, n_ep = 0, out_pos = 0;
    int rc = NFAGG_OK;
    const char* base = static_cast<const char*>(d_records);
    char* obase = static_cast<char*>(d_out);
    auto evict_pending = [&]() -> int {                         // the map is full and the record that found it so is next (account.go:85-94)
        if (n_ep >= max_epochs) return NFAGG_TRUNCATED;
        size_t got = 0;
        const int r = evict_core(h, NFAGG_REASON_FULL, obase + out_pos * kRecordBytes, true, out_cap - out_pos, &got);
        if (r != NFAGG_OK) return r;                            // NFAGG_TRUNCATED: nothing evicted, the caller drains `out` and calls again
        out_pos += got;
        epoch_end[n_ep++] = out_pos;
        return NFAGG_OK;
    };
    if (h->must_evict && n) rc = evict_pending();
    bool par_declined = false;
    while (rc == NFAGG_OK && consumed < n) {
        if (!par_declined && account_par_ok(h, n - consumed, out_cap - out_pos) && n_ep < max_epochs) {
            // the epochs of the call found first, then folded all at once (this file)
            size_t c = 0, e = 0, o = 0; uint32_t stop = 0;
            rc = account_par_launch(h, base + consumed * kRecordBytes, n - consumed, obase + out_pos * kRecordBytes, out_cap - out_pos,
                                    epoch_end + n_ep, max_epochs - n_ep, &c, &e, &o, &stop);
            for (size_t k = 0; k < e; k++) epoch_end[n_ep + k] += out_pos;
            consumed += c; n_ep += e; out_pos += o;
            if (rc == kParDeclined) { rc = NFAGG_OK; par_declined = true; h->stats.account_declined++; continue; }
            if (rc == NFAGG_OK) h->stats.account_epochs_first++;
            if (rc != NFAGG_OK) break;
            if (stop == 2) { rc = NFAGG_TRUNCATED; break; }
            continue;
        }
        if (account_fast_ok(h, n - consumed, out_cap - out_pos) && n_ep < max_epochs) {
            size_t c = 0, e = 0, o = 0; uint32_t stop = 0;
            h->stats.account_chain++;
            rc = account_chain_launch(
                h, base + consumed * kRecordBytes, n - consumed, obase + out_pos * kRecordBytes, out_cap - out_pos,
                epoch_end + n_ep, max_epochs - n_ep, &c, &e, &o, &stop);
            if (rc != NFAGG_OK) break;
            for (size_t k = 0; k < e; k++) epoch_end[n_ep + k] += out_pos;
            consumed += c; n_ep += e; out_pos += o;
            if (stop == 2) { rc = NFAGG_TRUNCATED; break; }     // no room for another eviction
            if (stop != 3) continue;                            // 3: the epoch tags wrap at the next eviction — that epoch goes through the host path below
        }
        size_t c = 0;
        rc = ingest_device_core(h, base + consumed * kRecordBytes, n - consumed, &c);
        consumed += c;
        if (rc == NFAGG_FULL) rc = evict_pending();
    }
    if (n_epochs_out) *n_epochs_out = n_ep;
    if (consumed_out) *consumed_out = consumed;
    return rc;
}

extern "C" {

int nfagg_account_device(nfagg_handle* h, const void* d_records, size_t n, void* d_out, size_t out_cap, uint64_t* epoch_end,
                         size_t max_epochs, size_t* n_epochs, size_t* consumed) {
    if (!h || (!d_records && n) || !epoch_end || !n_epochs || !consumed || (!d_out && out_cap)) return fail(h, NFAGG_EINVAL, "null argument");
    if ((((uintptr_t)d_records | (uintptr_t)d_out) & 15u) != 0) return fail(h, NFAGG_EINVAL, "device buffers must be 16-byte aligned");
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = account_device_core(h, d_records, n, d_out, out_cap, epoch_end, max_epochs, n_epochs, consumed);
    // synchronous, as the header says: the last launches of the call (k_finalize copies the new flows' identity dwords out of
    // d_records; a fall-through to the plain fold is asynchronous altogether) have read the caller's buffer when it returns
    if (rc >= 0) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return rc;
}

int nfagg_account(nfagg_handle* h, const void* records, size_t n, void* out, size_t out_cap, uint64_t* epoch_end, size_t max_epochs,
                  size_t* n_epochs_out, size_t* consumed_out) {
    if (!h || (!records && n) || !epoch_end || !n_epochs_out || !consumed_out || (!out && out_cap)) return fail(h, NFAGG_EINVAL, "null argument");
    if (h->stage_acquired) return fail(h, NFAGG_ESTATE, "a staging buffer is acquired; commit it first");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = staging_alloc(h);
    if (rc != NFAGG_OK) return rc;
    const char* src = static_cast<const char*>(records);
    const size_t cap = (size_t)h->cfg.staging_records;
    size_t consumed = 0, n_ep = 0, out_pos = 0;
    // Pinned ring, double buffered as in nfagg_ingest: chunk k+1 is copied into its pinned buffer and sent up on the copy
    // stream while the device works on chunk k. A chunk that stops early (no room for another eviction) ends the call.
    // The first chunks are short (a quarter, then half a staging buffer): nothing overlaps the first upload, so it should not be a
    // whole buffer's (2.6 ms of a 20 ms call for 8 M records over a 57 GB/s link).
    size_t staged_lo[2] = {0, 0}, staged_n[2] = {0, 0};
    const bool pinned_src = host_is_pinned(records);            // page-locked caller buffer: sent up as it is, no host copy
    const bool pinned_out = out_cap != 0 && host_is_pinned(out); // page-locked output: the evictions come down by DMA, asynchronously
    size_t n_staged = 0;
    // A call of about one staging buffer (the shim's batch: up to 1 Mi records) goes in up to four equal pieces, none shorter than
    // the epochs-found-first path takes: the first upload is a quarter of the call, the others overlap the device's work
    // (4.6 -> ~3.4 ms per 1 Mi-record call, profiles/r06_account_small_calls.txt).
    const size_t par_min = (size_t)account_par_min_records(h->cfg.max_entries);
    size_t piece = n;
    {
        size_t k = 4;
        while (k > 1 && n / k < (par_min > 131072 ? par_min : (size_t)131072)) k--;
        piece = ((n + k - 1) / k + 63) & ~(size_t)63;
    }
    auto stage = [&](int b, size_t lo) -> int {
        size_t want = cap;
        if (n > cap + cap / 2) { if (n_staged < 2) want = cap >> (2 - n_staged); }  // a long call ramps up: cap / 4, cap / 2, cap, cap, ...
        else want = piece;                                                          // a call of about one staging buffer: in up to four equal pieces
        // (never so short that the chunk leaves the epochs-found-first path, nor longer than a staging buffer)
        if (want < par_min) want = par_min;
        if (want > cap) want = cap;
        n_staged++;
        const size_t m = (n - lo) < want ? (n - lo) : want;
        HIP_TRY(h, hipEventSynchronize(h->stage_free[b]));
        const void* up = src + lo * kRecordBytes;
        if (!pinned_src) { staged_copy(h->pinned[b].p, up, m * kRecordBytes, h->cfg.copy_threads); up = h->pinned[b].p; }
        HIP_TRY(h, hipMemcpyAsync(h->d_stage[b].p, up, m * kRecordBytes, hipMemcpyHostToDevice, h->copy_stream));
        HIP_TRY(h, hipEventRecord(h->stage_up[b], h->copy_stream));
        staged_lo[b] = lo; staged_n[b] = m;
        return NFAGG_OK;
    };
    int b = h->stage_next;
    if (n && (rc = stage(b, 0)) != NFAGG_OK) return rc;
    // Three things overlap per chunk k: this thread drives the device over chunk k (synchronous); the evictions of chunk k-1
    // come down into the caller's buffer; chunk k+1 goes up. Two device buffers take the evictions in turn; a chunk of m records
    // delivers at most m + max_entries flows.
    //   page-locked output: an asynchronous copy on a stream of its own, waited for only when its device buffer comes round
    //     again (a blocking hipMemcpy from a helper thread was served only after the upload in flight: 3 ms of every second
    //     chunk, 27.6 ms for the 8 M-record call where the link needs 20.2 — profiles/r05_account_host_pipeline.txt);
    //   pageable output: a helper thread (pinned bounce buffers + host copies, d2h_copy).
    if (pinned_out) {
        if (!h->d2h_stream) HIP_TRY(h, h->d2h_stream.create());
        for (int k = 0; k < 2; k++)
            if (!h->bounce_ev[k]) HIP_TRY(h, h->bounce_ev[k].create());
    }
    bool down_pending[2] = {false, false};                      // pinned_out: a download from eviction buffer [k] is in flight
    struct { bool has = false; const void* d = nullptr; size_t got = 0, at = 0; } prev;
    auto bring_down = [&]() -> int {
        int rd = NFAGG_OK;
        if (prev.has && prev.got) rd = d2h_copy(h, (char*)out + prev.at * kRecordBytes, prev.d, prev.got * kRecordBytes);
        prev.has = false;
        return rd;
    };
    int ebuf = 0;
    while (rc == NFAGG_OK && consumed < n) {
        const size_t lo = staged_lo[b], m = staged_n[b];
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->stage_up[b], 0));
        const bool more = lo + m < n;
        size_t room = out_cap - out_pos;
        // a chunk of m records delivers at most max_entries + m flows, and the device loop wants room for one more whole eviction
        // (max_entries) whenever an epoch ends: with less it would report "no room" although the caller's buffer has some
        if (room > m + 2 * (size_t)h->cfg.max_entries) room = m + 2 * (size_t)h->cfg.max_entries;
        DevBuf& dbuf = ebuf ? h->d_ep_out : h->d_evict;
        if (down_pending[ebuf]) { HIP_TRY(h, hipEventSynchronize(h->bounce_ev[ebuf])); down_pending[ebuf] = false; }   // its last download has left
        if ((rc = dbuf.ensure(h, room * kRecordBytes + 16)) != NFAGG_OK) break;
        size_t c = 0, e = 0;
        int rc_helper = NFAGG_OK, rc_helper2 = NFAGG_OK;
        std::thread helper, helper2;                            // one brings chunk k-1's evictions down (pageable output), one sends chunk k+1 up
        const bool down = !pinned_out && prev.has && prev.got != 0;
        // (a thread that cannot be created must not throw through the C boundary: its job is done here and now instead)
        auto spawn = [](std::thread& t, auto fn) { try { t = std::thread(fn); } catch (...) { fn(); } };
        if (down) spawn(helper, [&] { (void)hipSetDevice(h->device); rc_helper = bring_down(); });
        else prev.has = false;
        if (more) spawn(helper2, [&] { (void)hipSetDevice(h->device); rc_helper2 = stage(b ^ 1, lo + m); });
        NF_DIAG_T(t_a);
        rc = account_device_core(h, h->d_stage[b].p, m, dbuf.p, room, epoch_end + n_ep, max_epochs - n_ep, &e, &c);
        NF_DIAG_T(t_b);
        if (helper.joinable()) helper.join();
        NF_DIAG_T(t_c);
        if (helper2.joinable()) helper2.join();
        NF_DIAG_T(t_d);
        NF_DIAG_PRINT("[account] chunk at %zu: %zu records, core %.2f ms (%zu evictions), wait down %.2f, wait up %.2f\n", lo, m, t_b - t_a, e, t_c - t_b, t_d - t_c);
        if (rc_helper == NFAGG_OK) rc_helper = rc_helper2;
        if (rc == NFAGG_OK && rc_helper != NFAGG_OK) rc = rc_helper;
        HIP_TRY(h, hipEventRecord(h->stage_free[b], h->stream));
        const size_t got = e ? (size_t)epoch_end[n_ep + e - 1] : 0;
        if (pinned_out) {
            if (got && rc >= 0) {
                // account_device_core has synchronised the fold stream for everything it wrote into dbuf.p
                HIP_TRY(h, hipStreamSynchronize(h->stream));
                HIP_TRY(h, hipMemcpyAsync((char*)out + out_pos * kRecordBytes, dbuf.p, got * kRecordBytes, hipMemcpyDeviceToHost, h->d2h_stream));
                HIP_TRY(h, hipEventRecord(h->bounce_ev[ebuf], h->d2h_stream));
                down_pending[ebuf] = true;
            }
        } else {
            prev.has = true; prev.d = dbuf.p; prev.got = got; prev.at = out_pos;
        }
        for (size_t k = 0; k < e; k++) epoch_end[n_ep + k] += out_pos;
        n_ep += e; out_pos += got; consumed += c;
        h->stage_next = b ^ 1;
        ebuf ^= 1;
        if (rc != NFAGG_OK || c < m) break;                     // stopped inside the chunk: what was staged beyond it is staged again by the next call
        b ^= 1;
    }
    {
        int rc_down = bring_down();
        if (pinned_out && (down_pending[0] || down_pending[1]) && hipStreamSynchronize(h->d2h_stream) != hipSuccess)
            rc_down = fail(h, NFAGG_EDEVICE, "eviction download failed");
        if (rc == NFAGG_OK || rc == NFAGG_TRUNCATED) { if (rc_down != NFAGG_OK) rc = rc_down; }
    }
    if (pinned_src) (void)hipStreamSynchronize(h->copy_stream);       // a chunk staged ahead may still be on its way: the caller's buffer is its own again
    *n_epochs_out = n_ep; *consumed_out = consumed;
    return rc;
}

}  // extern "C"
