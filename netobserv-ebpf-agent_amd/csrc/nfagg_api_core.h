// nfagg_api_core.h — what nfagg_api.hip (the flow table: fold, eviction, partials, the staging ring) offers the two files that
// drive a handle through its internals: nfagg_api_account.hip (nfagg_account*) and nfagg_api_group.hip (the multi-GPU group).
// All of it is defined in nfagg_api.hip and documented there. Private to csrc/; nfagg.map exports nothing of it.
#pragma once
#include "nfagg_handle.h"

namespace nfagg {

extern const uint64_t kSeqWindow;        // relative sequence numbers stay below this
extern const uint64_t kMaxFoldChunk;     // records per pass of the ingest loop

// profiling
void prof_begin(nfagg_handle* h, EventPair& ep, int kind);
void prof_end(nfagg_handle* h, EventPair& ep);
void prof_resolve(nfagg_handle* h);

// the fold and its bookkeeping
int launch_ingest_profiled(nfagg_handle* h, const void* d, uint64_t n, uint64_t seq_base);
int refresh_counters_enqueue(nfagg_handle* h);
int refresh_counters_taken(nfagg_handle* h);
int refresh_counters(nfagg_handle* h);
int ensure_seq_window(nfagg_handle* h, uint64_t n, bool* blocked);
int ingest_device_core(nfagg_handle* h, const void* d_records, size_t n, size_t* consumed_out);
int evict_core(nfagg_handle* h, int reason, void* out, bool out_is_device, size_t cap, size_t* n_out);

// the pieces of an optimistic fold
struct OptState {
    uint64_t old_live = 0, seq0 = 0, room = 0, n_after = 0;
    DevCounters before{};
    bool was_unclustered = false;
};
int opt_begin(nfagg_handle* h, OptState& st);
int opt_fold(nfagg_handle* h, const OptState& st, const void* d, uint64_t chunk);
int opt_result(nfagg_handle* h, OptState& st, uint64_t chunk, bool* crossed, bool* aborted, uint64_t* split);
void opt_commit(nfagg_handle* h, const OptState& st, uint64_t chunk);
int opt_rollback(nfagg_handle* h, const OptState& st);

// the staging ring and the copies to and from host memory
int staging_alloc(nfagg_handle* h);
size_t stage_chunk(const nfagg_handle* h, size_t remaining, size_t cap);
void staged_copy(void* dst, const void* src, size_t bytes, unsigned threads);
bool host_is_pinned(const void* p);
int d2h_copy(nfagg_handle* h, void* dst, const void* d_src, size_t bytes);

// local fold across GPUs
int partials_export_core(nfagg_handle* h, uint32_t n_shards, uint32_t self_shard, void* d_out, size_t cap, uint64_t* counts, size_t* n_out);
int partials_merge_core(nfagg_handle* h, uint32_t n_shards, uint32_t shard_id, const void* d_partials, size_t n);
int owned_count_core(nfagg_handle* h, uint32_t n_shards, uint32_t shard_id, uint64_t* owned, uint64_t* claimed_out);
int evict_owned_core(nfagg_handle* h, int reason, uint32_t n_shards, uint32_t shard_id, void* d_out, size_t cap, size_t* n_out);
int window_clear_core(nfagg_handle* h);
int window_finish_core(nfagg_handle* h, uint64_t next_seq);

}  // namespace nfagg
