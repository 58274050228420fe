// nfagg_handle.h — what the host translation units of the C ABI share (nfagg_api.hip: the flow table; nfagg_api_account.hip:
// nfagg_account*; nfagg_api_group.hip: the multi-GPU group; nfagg_api_export.hip, nfagg_api_tables.hip, nfagg_api_filter.hip,
// nfagg_api_conn.hip, nfagg_api_loki.hip, nfagg_api_flp_ipfix.hip, nfagg_api_aux.hip: the encoders, the caller tables, the writers,
// the side operations; what their entry points do alike is nfagg_api_call.h): error reporting, the owner types
// — every device / pinned allocation, stream, event and graph of the library lives in one and is released by its destructor —
// and the handle behind nfagg_handle*, which holds nothing but owners and plain state: `delete h` frees all of it.
// Private to csrc/; nothing here is exported (nfagg.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/nfagg.h"
#include "nfagg_internal.h"

namespace nfagg {

// Sets the handle's error text (without a handle: the calling thread's create error, nfagg_last_error(NULL)) and returns `code`.
// Defined once, in nfagg_api.hip, beside the create-error string: every translation unit reports into the same one.
int fail(nfagg_handle* h, int code, const char* fmt, ...);

inline uint64_t next_pow2(uint64_t v) { uint64_t p = 1; while (p < v) p <<= 1; return p; }

// Device and pinned allocations of this library that are alive (nfagg_debug_live_buffers): counted where they are made and freed
inline std::atomic<uint64_t> g_live_buffers{0};

// Device memory (DevBuf) and page-locked host memory (PinnedBuf). alloc: a fixed size, once (flags: as hipHostMalloc takes them,
// page-locked memory only). ensure: grow-only scratch — at least `need` bytes afterwards; the contents do not survive a growth
// (the old block is freed first; the new one has 4 KiB to spare, device memory a quarter more).
template <bool kPinned> struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ~Buf() { reset(); }
    void reset() { if (p) { (void)(kPinned ? hipHostFree(p) : hipFree(p)); g_live_buffers--; p = nullptr; cap = 0; } }
    hipError_t alloc(size_t bytes, unsigned flags = hipHostMallocDefault) {
        reset();
        const hipError_t e = kPinned ? hipHostMalloc(&p, bytes, flags) : hipMalloc(&p, bytes);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = bytes; g_live_buffers++;
        return hipSuccess;
    }
    int ensure(nfagg_handle* h, size_t need) { return cap >= need ? NFAGG_OK : grow(h, need); }
    int grow(nfagg_handle* h, size_t need) {
        const size_t want = need + (kPinned ? 0 : need / 4) + 4096;
        const hipError_t e = alloc(want);
        return e == hipSuccess ? NFAGG_OK : fail(h, kPinned ? NFAGG_EDEVICE : NFAGG_ENOMEM, "%s(%zu) failed: %s", kPinned ? "hipHostMalloc" : "hipMalloc", want, hipGetErrorString(e));
    }
    template <typename T> T* as() const { return static_cast<T*>(p); }
    explicit operator bool() const { return p != nullptr; }
};
using DevBuf = Buf<false>;
using PinnedBuf = Buf<true>;

// A stream, an event, an instantiated graph: created on first use by the code that needs them, read through the conversion.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create(unsigned flags = hipStreamNonBlocking) { return hipStreamCreateWithFlags(&s, flags); }
    operator hipStream_t() const { return s; }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDisableTiming) { return hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};
struct GraphExec {
    hipGraphExec_t g = nullptr;
    GraphExec() = default;
    GraphExec(GraphExec&& o) noexcept : g(o.g) { o.g = nullptr; }
    ~GraphExec() { reset(); }
    void reset() { if (g) { (void)hipGraphExecDestroy(g); g = nullptr; } }
    operator hipGraphExec_t() const { return g; }
};

struct EventPair { hipEvent_t a, b; int kind; };     // borrowed from nfagg_handle::ev_pool

// The arrays a TableView points into
struct TableMem { DevBuf hot, cold, aux, live_list, ctr; };

// The export encoders (protobuf, IPFIX, direct-FLP JSON), write ipfix, the filter, conntrack, the resolves and the metrics folds:
// one scratch, they serialise on the stream and synchronise before returning. Who stages what (nfagg_api_call.h):
struct EncodeScratch {
    DevBuf local_off, block_sum, block_base;     // encode_begin: the two scans, u32[n], u32[blocks], u64[blocks + 1] (the total last);
                                                 //   the filter, the conversation fold and the metrics folds size them for their own scans
    DevBuf names;                                // stage_namer: the namer table, stably sorted by if_index (write ipfix's too)
    DevBuf ipfix_name_rows;                      // size pass -> write pass: u32[n]
    DevBuf flp_rows;                             // size pass -> write pass: 8 x u32 per record (seven rows, the line's length)
    DevBuf flp_esc, flp_n_deferred;              // the escaped table; the deferred counter
    DevBuf in_records, out, out_offsets;         // encode_staged and the other twins: staged records, output bytes, offsets (the filter
                                                 //   and the gather: kept indexes)
    DevBuf out_extra[2];                         //   protobuf: body lengths, kafka keys; FLP: deferred flags; write ipfix: status bytes;
                                                 //   the filter: keep and rule bytes
    DevBuf pb_feat[6];                           //   stage_pb_features: present bits and the five feature parts
    DevBuf ne_rows;                              //   *_netev: the flows' table rows
    DevBuf ne_in[3], ne_out[3], ne_missing, ne_info;   // nfagg_netev_resolve: staged inputs and outputs, the missing set, its counters
    DevBuf k8s_rows;                             // *_k8s and nfagg_k8s_resolve: the flows' two table rows, 2 x u32 per record; staged there
                                                 //   by the twins that take them from the caller (net resolve, filter, metrics, write ipfix)
    DevBuf net_rows;                             // *_net and nfagg_net_resolve: the flows' nfagg_net_row, 8 bytes per record; staged likewise
    DevBuf met_slots, met_out;                   // nfagg_metrics_fold: control words and the groupings' tables; the host entry point's groups
    DevBuf conn_slots, conn_flow;                // nfagg_conn_fold: control words and the connection table; per flow hashA and slot
    DevBuf conn_ids, conn_out;                   //   the host entry point's hash ids and partials; the host entry points of the two
                                                 //   conntrack encoders stage their ids / values here too (one stream: calls serialise)
    std::vector<nfagg_intf_name> h_names;        // stage_namer's and stage_flp_line's host copies, kept until the stream has consumed them
    std::vector<uint8_t> h_flp_esc;
};

// nfagg_rollup_*
struct RollupScratch { DevBuf partials, base, folded; };

// nfagg_map_merge*: the join's slots and scans; the host variant's staged maps (main map, then the six feature maps) and outputs
struct MergeScratch {
    DevBuf slots, slot_of, local_off, block_sum, block_base, n_dup;
    DevBuf ids[7], vals[7], out[8];
};

// nfagg_cm_topk*
struct TopkScratch { DevBuf est, est_sorted, idx, idx_sorted, sort_tmp, rows, records; };    // records: the host variant's

// optimistic fold: raw slot snapshot, sketch snapshot, first sequence numbers (+ sorted), sort scratch
struct OptScratch { DevBuf slots, sketches, first_seqs, sort_tmp; };

// nfagg_loki_plan / nfagg_loki_write (nfagg_api_loki.hip): the plan's arrays and state, kept until the next plan. Defined there;
// the handle owns it through the deleter that file installs.
struct LokiPlan;

// nfagg_account*, the kernel chain: control block, epoch ends, live-list scratch (device); pinned: control block, then the epoch ends
struct ChainScratch { DevBuf ctl, ends, live; PinnedBuf host; };

// nfagg_account*, the epochs found first (nfagg_api_account.hip): the analysis arrays, the pinned control words and cuts, the stream
// the middle epochs are folded on while the table takes the first and the last
struct ParScratch {
    DevBuf keys, keys_sorted, prev, pos, long_segs, sort_tmp, ctl, rank_tiles;   // ctl: control words, then the cuts
    PinnedBuf host;                     // control words, the cuts, the walk parts' state
    Stream stream;
    Event done;
    Event part[16];                     // one behind every part of the cut walk (kParWalkPartsMax)
};

}  // namespace nfagg

struct nfagg_handle {
    nfagg_config cfg{};
    int device = 0;
    // streams first: destroyed after everything that was used on them
    nfagg::Stream stream;
    nfagg::Stream copy_stream;      // H2D copies of the staging ring: chunk k+1 goes up while chunk k is folded on `stream`
    nfagg::Stream d2h_stream;
    nfagg::Stream d2h_small;        // small / one-off downloads (d2h_copy): not the stream the pipelined page-locked downloads use
    uint64_t slots = 0;
    nfagg::TableView tv{};          // points into `table`, `spill_queues`, `spill_xp`, `qtail`
    nfagg::TableMem table;
    nfagg::SketchView sk{};         // points into `sketch` or at the caller's buffers (cfg.ext_sketch)
    nfagg::DevBuf sketch[4];        // Count-Min src, dst; HyperLogLog src, dst — the ones the caller did not supply
    nfagg::PinnedBuf ctr_mirror; nfagg::DevCounters* h_ctr = nullptr;        // the counters' pinned mirror, and how the code reads it
    // staging ring (host ingest path)
    nfagg::PinnedBuf pinned[2];
    nfagg::DevBuf d_stage[2];
    nfagg::Event stage_free[2], stage_up[2];
    int stage_next = 0;
    bool stage_acquired = false;
    // careful-path scratch
    uint64_t careful_chunk = 0;
    nfagg::DevBuf d_slot_idx, d_flags, d_block_counts;
    std::vector<uint32_t> h_block_counts;
    nfagg::PinnedBuf careful_mirror; uint8_t* h_careful = nullptr;   // block counts + flags of a claim + flag chunk of up to kCarefulMaxBatch records
    nfagg::DevBuf d_evict;          // eviction buffer (device)
    nfagg::DevBuf d_ep_out;         // second device buffer for evictions (nfagg_account alternates with d_evict)
    nfagg::RollupScratch roll;
    nfagg::DevBuf d_hist;
    nfagg::MergeScratch mm;
    nfagg::TopkScratch hh;
    nfagg::DevBuf sort_live, sort_tmp;   // eviction: live list in slot order, radix-sort scratch
    int sort_bits = 0;
    bool epoch_unclustered = false; // a batch of this epoch claimed slots in arrival order (single-pass / direct / dedup kernels)
    nfagg::EncodeScratch enc;
    nfagg::OptScratch opt;
    std::unique_ptr<nfagg::LokiPlan, void (*)(nfagg::LokiPlan*)> loki{nullptr, nullptr};
    uint64_t epoch_len_hint = 0;   // records the last epoch that ended on "full" took (0 = this stream has not stopped on full)
    uint64_t last_epoch_flows = 0; // slots the last epoch had claimed when it ended (flows; sub-flows on a sub-flow table): what the next one is sized by
    uint64_t abort_cap = 0;        // largest chunk worth trying after the kernels refused claims (0 = no limit known)
    // spill queues of the two-pass ingest: partition queues + overflow list; the streaming pass's exported cache entries; the tails
    nfagg::DevBuf spill_queues, spill_xp, qtail;
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
    bool must_evict = false; // a "full" split is pending (account.go:85-94)
    uint64_t split_seq = 0;
    // local fold across GPUs (nfagg_partials_*): the flows of other shards have been exported to their owners; nothing may be
    // folded on top of them before the eviction (they would be exported twice)
    bool exported = false;
    nfagg::DevBuf d_exp;            // 64 owner counts + 64 segment cursors + the owned-flows count
    nfagg::PinnedBuf exp_mirror; unsigned long long* h_exp = nullptr;   // pinned mirror of the counts
    nfagg::ChainScratch chain;
    // device -> pageable host memory through two pinned bounce buffers (d2h_copy): a plain hipMemcpy to pageable memory runs at
    // ~13 GB/s here, this at the PCIe rate
    nfagg::PinnedBuf h_bounce[2];
    nfagg::Event bounce_ev[2];
    nfagg::GraphExec ep_graph[3];        // kChainWindows[k] windows of the epoch kernel chain, captured once (their arguments never change)
    bool ep_graph_off = false;           // the capture or the instantiation failed once: this handle launches its windows eagerly
    void* ep_graph_key[3] = {};          // the buffers the captured launches point at: re-capture when one was re-allocated
    // sub-flow table (kernel-dedup mode of a local-fold rank, nfagg_dedup.h): the flow-keyed table its epochs are joined into
    // (nfagg_dedup_join.hip), allocated at the first eviction; scratch; the join that has been made and not yet evicted
    nfagg::TableView jv{};          // points into `jtable`
    nfagg::TableMem jtable;
    nfagg::PinnedBuf jctr_mirror; nfagg::DevCounters* h_jctr = nullptr;   // pinned mirror of jv.ctr
    nfagg::DevBuf d_join;           // slot_of[]: the J slot of every live sub-flow
    struct { bool valid = false, dirty = false; uint32_t n_shards = 0, shard_id = 0; uint64_t flows = 0, claimed = 0; } join;   // dirty: J may hold claims
    nfagg::ParScratch par; uint32_t* h_par = nullptr;           // (h_par: par.host as the code reads it)
    nfagg_stats stats{};
    std::vector<nfagg::Event> ev_pool;        // profiling: every event ever created for this handle
    std::vector<nfagg::EventPair> ev_pending;
    std::vector<nfagg::EventPair> ev_free;
    std::mutex err_mu;              // nfagg_account's helper threads report through fail() too
    std::string err;
};

// The end of an object that lives on a handle's device (caller tables, filters, layouts): the handle's stream may still be reading
// its buffers, so it is waited for; the object's owners free them.
template <typename T> void destroy_on_handle(T* t) {
    if (!t) return;
    if (t->h) { (void)hipSetDevice(t->h->device); (void)hipStreamSynchronize(t->h->stream); }
    delete t;
}

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
