// nfagg_handle.h — what the host translation units of the C ABI share (nfagg_api.hip: the flow table; nfagg_api_export.hip,
// nfagg_api_tables.hip, nfagg_api_aux.hip: the encoders, the caller tables, the side operations): the handle behind
// nfagg_handle*, error reporting, the grow-only device buffers. Private to csrc/; nothing here is exported (nfagg.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"

namespace nfagg {

struct EventPair { hipEvent_t a, b; int kind; };

}  // namespace nfagg

struct nfagg_handle {
    nfagg_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t slots = 0;
    nfagg::TableView tv{};
    nfagg::SketchView sk{};
    bool own_sketch[4] = {false, false, false, false};
    nfagg::DevCounters* h_ctr = nullptr;      // pinned mirror
    // staging ring (host ingest path)
    void* pinned[2] = {nullptr, nullptr};
    void* d_stage[2] = {nullptr, nullptr};
    hipEvent_t stage_free[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr;   // H2D copies of the staging ring: chunk k+1 goes up while chunk k is folded on `stream`
    hipEvent_t stage_up[2] = {nullptr, nullptr};
    int stage_next = 0;
    bool stage_acquired = false;
    // careful-path scratch
    uint64_t careful_chunk = 0;
    uint32_t* d_slot_idx = nullptr;
    uint8_t* d_flags = nullptr;
    uint32_t* d_block_counts = nullptr;
    std::vector<uint32_t> h_block_counts;
    // eviction buffer (device)
    void* d_evict = nullptr;
    uint64_t d_evict_cap = 0;
    // rollup scratch
    void* d_roll[3] = {nullptr, nullptr, nullptr};
    size_t d_roll_cap[3] = {0, 0, 0};
    uint32_t* d_hist = nullptr;
    // map merge scratch: [0] slots [1] slot_of [2] local_off [3] block_sum [4] block_base [5] dup counter,
    // (host variant) [6..12] ids, [13..19] values, [20..27] outputs
    void* d_mm[28] = {};
    size_t d_mm_cap[28] = {};
    void* d_hh[7] = {};            // heavy hitters: est, est sorted, idx, idx sorted, sort scratch, gathered rows, (host variant) records
    size_t d_hh_cap[7] = {};
    void* d_sort[2] = {};          // eviction: live list in slot order, radix-sort scratch
    size_t d_sort_cap[2] = {};
    int sort_bits = 0;
    bool epoch_unclustered = false; // a batch of this epoch claimed slots in arrival order (single-pass / direct / dedup kernels)
    // export encoders (protobuf, IPFIX, direct-FLP JSON): one scratch, they serialise on the stream and synchronise before returning
    struct DevBuf { void* p = nullptr; size_t cap = 0; };
    struct EncodeScratch {
        DevBuf local_off, block_sum, block_base;     // the two scans: u32[n], u32[blocks], u64[blocks + 1] (the total last)
        DevBuf names;                                // the namer table, stably sorted by if_index
        DevBuf ipfix_name_rows;                      // size pass -> write pass: u32[n]
        DevBuf flp_rows;                             // size pass -> write pass: 8 x u32 per record (seven rows, the line's length)
        DevBuf flp_esc, flp_n_deferred;              // the escaped table; the deferred counter
        DevBuf in_records, out, out_offsets;         // host-memory entry points: staged records, output bytes, offsets
        DevBuf out_extra[2];                         //   protobuf: body lengths, kafka keys; FLP: deferred flags
        DevBuf pb_feat[6];                           //   protobuf: present bits and the five feature parts
        DevBuf ne_rows;                              //   *_netev: the flows' table rows
        DevBuf ne_in[3], ne_out[3], ne_missing, ne_info;   // nfagg_netev_resolve: staged inputs and outputs, the missing set, its counters
        DevBuf k8s_rows;                             // *_k8s and nfagg_k8s_resolve: the flows' two table rows, 2 x u32 per record
        DevBuf net_rows;                             // *_net and nfagg_net_resolve: the flows' nfagg_net_row, 8 bytes per record
        DevBuf met_slots, met_out;                   // nfagg_metrics_fold: control words and the groupings' tables; the host entry point's groups
        DevBuf conn_slots, conn_flow;                // nfagg_conn_fold: control words and the connection table; per flow hashA and slot
        DevBuf conn_ids, conn_out;                   //   the host entry point's hash ids and partials; the host entry points of the two
                                                     //   conntrack encoders stage their ids / values here too (one stream: calls serialise)
        std::vector<nfagg_intf_name> h_names;        // host copies, kept until the stream has consumed them
        std::vector<uint8_t> h_flp_esc;
        template <typename F> void each(F f) {
            for (DevBuf* b : {&local_off, &block_sum, &block_base, &names, &ipfix_name_rows, &flp_rows, &flp_esc, &flp_n_deferred,
                              &in_records, &out, &out_offsets, &out_extra[0], &out_extra[1]}) f(*b);
            for (DevBuf& b : pb_feat) f(b);
            for (DevBuf* b : {&ne_rows, &ne_in[0], &ne_in[1], &ne_in[2], &ne_out[0], &ne_out[1], &ne_out[2], &ne_missing, &ne_info, &k8s_rows, &net_rows, &met_slots, &met_out,
                              &conn_slots, &conn_flow, &conn_ids, &conn_out}) f(*b);
        }
    } enc;
    // optimistic fold: [0] raw slot snapshot, [1] sketch snapshot, [2] first sequence numbers (+ sorted), [3] sort scratch
    void* d_opt[4] = {};
    size_t d_opt_cap[4] = {};
    uint64_t epoch_len_hint = 0;   // records the last epoch that ended on "full" took (0 = this stream has not stopped on full)
    uint64_t last_epoch_flows = 0; // slots the last epoch had claimed when it ended (flows; sub-flows on a sub-flow table): what the next one is sized by
    uint64_t abort_cap = 0;        // largest chunk worth trying after the kernels refused claims (0 = no limit known)
    // spill queues of the two-pass ingest
    void* d_spill = nullptr;
    size_t d_spill_cap = 0;
    // accounting
    uint64_t epoch_seq = 0;         // sequence number of the next record, counted from the start of the epoch (64 bits: never runs out)
    uint64_t seq_origin = 0;        // the device sees epoch_seq - seq_origin: a 32-bit window, moved by a rebase (nfagg_rebase.hip)
    bool ext_sequenced = false;     // sequence numbers are handed in (nfagg_set_sequence, group local fold): other tables hold tags of the
                                    // same numbering, so this handle must not move its window on its own
    uint64_t live = 0;       // len(entries): exact after refresh_counters and on the paths that keep counters_exact
    uint64_t live_ub = 0;    // upper bound on the device's n_live (the claimed slots); equal to it while counters_exact
    // The host knows the device's n_live and len(entries) without asking (after an eviction; after a claim + flag chunk,
    // whose counts it has just read): the next "might this batch fill the table" / eviction needs no round trip. Every
    // asynchronous fold clears it. mirror_fresh: *h_ctr equals the device counters (what the optimistic fold's rollback restores).
    bool counters_exact = false;
    bool mirror_fresh = false;
    uint8_t* h_careful = nullptr;   // pinned: block counts + flags of a claim + flag chunk of up to kCarefulMaxBatch records
    bool must_evict = false; // a "full" split is pending (account.go:85-94)
    uint64_t split_seq = 0;
    // local fold across GPUs (nfagg_partials_*): the flows of other shards have been exported to their owners; nothing may be
    // folded on top of them before the eviction (they would be exported twice)
    bool exported = false;
    void* d_exp = nullptr;          // 64 owner counts + 64 segment cursors + the owned-flows count
    size_t d_exp_cap = 0;
    unsigned long long* h_exp = nullptr;   // pinned mirror of the counts
    // nfagg_account*: control block of the epoch kernel chain (device + pinned mirror), epoch ends, slot scratch
    void* d_ep[3] = {};             // [0] control block, [1] epoch ends, [2] live-list scratch
    size_t d_ep_cap[3] = {};
    void* d_ep_out = nullptr;       // second device buffer for evictions (nfagg_account alternates with d_evict)
    size_t d_ep_out_cap = 0;
    void* h_ep = nullptr;           // pinned: control block, then the epoch ends
    size_t h_ep_cap = 0;
    // device -> pageable host memory through two pinned bounce buffers (d2h_copy): a plain hipMemcpy to pageable memory runs at
    // ~13 GB/s here, this at the PCIe rate
    void* h_bounce[2] = {nullptr, nullptr};
    hipStream_t d2h_stream = nullptr;
    hipStream_t d2h_small = nullptr;     // small / one-off downloads (d2h_copy): not the stream the pipelined page-locked downloads use
    hipEvent_t bounce_ev[2] = {nullptr, nullptr};
    hipGraphExec_t ep_graph[3] = {nullptr, nullptr, nullptr};   // kChainWindows[k] windows of the epoch kernel chain, captured once (their arguments never change)
    bool ep_graph_off = false;           // the capture or the instantiation failed once: this handle launches its windows eagerly
    void* ep_graph_key[3] = {};          // the buffers the captured launches point at: re-capture when one was re-allocated
    // sub-flow table (kernel-dedup mode of a local-fold rank, nfagg_dedup.h): the flow-keyed table its epochs are joined into
    // (nfagg_dedup_join.hip), allocated at the first eviction; scratch; the join that has been made and not yet evicted
    nfagg::TableView jv{};
    nfagg::DevCounters* h_jctr = nullptr; // pinned mirror of jv.ctr
    void* d_join = nullptr;         // slot_of[]: the J slot of every live sub-flow
    size_t d_join_cap = 0;
    struct { bool valid = false, dirty = false; uint32_t n_shards = 0, shard_id = 0; uint64_t flows = 0, claimed = 0; } join;   // dirty: J may hold claims
    // the evict-on-full loop with its epochs found first (nfagg_account_par.inc): analysis arrays, pinned mirror, the stream the
    // middle epochs are folded on while the table takes the first and the last
    uint32_t* h_par = nullptr;      // pinned: control words, then the cuts
    void* d_par[8] = {};            // sort keys, sorted keys, prev, pos, long segments, sort scratch, control + cuts, rank tile counts
    size_t d_par_cap[8] = {};
    hipStream_t par_stream = nullptr;
    hipEvent_t par_done = nullptr;
    hipEvent_t par_part[16] = {};   // one behind every part of the cut walk (kParWalkPartsMax)
    nfagg_stats stats{};
    std::vector<nfagg::EventPair> ev_pending;
    std::vector<nfagg::EventPair> ev_free;
    std::mutex err_mu;              // nfagg_account's helper threads report through fail() too
    std::string err;
};

namespace nfagg {

// Sets the handle's error text (without a handle: the calling thread's create error, nfagg_last_error(NULL)) and returns `code`.
// Defined once, in nfagg_api.hip, beside the create-error string: every translation unit reports into the same one.
int fail(nfagg_handle* h, int code, const char* fmt, ...);

// Grow-only device scratch: (*p, *cap) holds at least `need` bytes afterwards; the contents do not survive a growth (nfagg_api.hip).
int ensure_bytes(nfagg_handle* h, void** p, size_t* cap, size_t need);
inline int ensure_buf(nfagg_handle* h, nfagg_handle::DevBuf& b, size_t need) { return ensure_bytes(h, &b.p, &b.cap, need); }

inline uint64_t next_pow2(uint64_t v) { uint64_t p = 1; while (p < v) p <<= 1; return p; }

}  // namespace nfagg

#define HIP_TRY(h, expr)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return nfagg::fail((h), NFAGG_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// ... with something to do before the error is reported (a second stream to join)
#define HIP_TRY_DO(h, expr, cleanup)                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            cleanup;                                                                          \
            return nfagg::fail((h), NFAGG_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
        }                                                                                     \
    } while (0)
