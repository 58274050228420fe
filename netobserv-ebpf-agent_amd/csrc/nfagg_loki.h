// nfagg_loki.h — flowlogs-pipeline's write loki on the device (include/nfagg.h, "write loki on the device"):
// what the kernels of nfagg_loki.hip and the host side in nfagg_api_loki.hip share. The reference:
//   pkg/pipeline/write/write_loki.go:223-251 splitLabelsLines, :253-277 extractTimestamp, write_stdout.go:42-51 the line
//   loki-client-go/loki/client.go:154-172 the cut rule, batch.go:39-54, 63-65, 96-107 streams of a batch
//   loki-client-go/pkg/logproto/types.go:88-144, timestamp.go:59-106 the three MarshalTo, validateTimestamp
// A call is a PLAN (one key kernel, the ranks of the streams, the batch cuts, a sort by (batch, stream), the groups) and a
// WRITE (sizes of the stream headers, the offsets, the write kernel, the headers). The plan's arrays stay on the handle.
#pragma once
#include "nfagg_flp.h"

namespace nfagg {

constexpr uint32_t kLokiMaxStreams = NFAGG_LOKI_MAX_STREAMS, kLokiLabelsMax = NFAGG_LOKI_LABELS_MAX;
// 0x12 len(3) | 0x0a len(1) | 0x08 seconds(10) 0x10 nanos(5) | 0x12 len(3): what an entry has around its line at most
constexpr uint32_t kLokiFrameMax = 1 + 3 + 1 + 1 + (1 + 10 + 1 + 5) + 1 + 3;
static_assert(kLokiFrameMax == 27, "entry framing");
constexpr uint32_t kLokiMinSlots = 1024;                       // the stream table: a power of two of at least this
constexpr uint64_t kLokiNoGroup = 1ull << 52;                  // the sort key of a flow that takes part in nothing
constexpr int kLokiStreamBits = 20;
static_assert((1u << kLokiStreamBits) == kLokiMaxStreams, "a sort key is batch << 20 | stream");
constexpr int64_t kLokiMinSeconds = -62135596800ll, kLokiMaxSeconds = 253402300800ll;      // timestamp.go:31-36

// The table of nfagg_loki_table_create on the device: the Kubernetes rows and blocks without the keys the stage takes out of
// the line (the shape of K8sDev's own), a class per row and side over the label fields, a canonical label per subnet label.
struct LokiDev {
    const K8sRow* rows;
    const uint8_t* blob;
    const uint32_t* cls[2];       // nullptr: no label field on that side
    const uint16_t* canon;        // per net label: the first label with the same text; 0xFFFF: empty or not valid UTF-8
    uint32_t label_keys, omit_keys;       // omit: label or ignored, gone from the line
    uint32_t ts_source;
    double ts_scale;
    int64_t now_sec, now_nsec;    // timeNow() as time.Time has it
};

// Control words of a plan (device memory; read back once).
struct LokiCtl {
    uint32_t n_streams, n_groups, n_batches, n_deferred;
    uint32_t n_part;              // flows that take part: a line, and not deferred
    uint32_t claimed, over;       // slots of the stream table in use; more than kLokiMaxStreams, or a table walked through
    uint32_t pad_;
};

// What the key kernel writes and the later ones read, per flow unless said otherwise.
struct LokiPlanDev {
    LokiCtl* ctl;
    uint64_t* keys;               // the stream table: two words per slot (claim protocol of nfagg_metrics.hip, two words)
    uint32_t* first;              // per slot: the first flow of the stream (atomic min)
    uint32_t* sid;                // per slot: the dense stream id
    uint32_t mask;
    uint32_t* slot_of;            // kNoSlot: takes part in nothing
    uint32_t* rows8;              // seven interface rows and the line's length (0: takes part in nothing)
    int64_t* ts;                  // seconds, nanos
    uint32_t* lens;               // the line's length again, for the scan
    uint8_t* deferred;
};

// Scratch of the 64-bit prefix sums: u32[count], u32[blocks], u64[blocks + 1] for the longest scan of a call (n + 1 values).
struct LokiScan { uint32_t* local_off; uint32_t* block_sum; uint64_t* block_base; };

// plan
// content: the flows carry feature parts (A.F); with A.F.ne_rows their network events too (nfagg_flp_content.hip's policies)
hipError_t launch_loki_key(const FlpLineArgs& A, bool content, const LokiDev& L, const LokiPlanDev& D, hipStream_t s);
hipError_t launch_loki_rank(uint64_t n, const LokiPlanDev& D, uint32_t* d_flag, uint32_t* d_rank, nfagg_loki_stream* d_streams, void* d_tmp,
                            size_t tmp_bytes, hipStream_t s);
hipError_t launch_loki_cuts(uint64_t n, const LokiPlanDev& D, uint64_t* d_pinc, uint32_t batch_size, uint32_t* d_cuts, const LokiScan& X, hipStream_t s);
hipError_t launch_loki_sort(uint64_t n, const LokiPlanDev& D, const uint32_t* d_cuts, uint64_t* d_key, uint64_t* d_key_sorted, uint32_t* d_val,
                            uint32_t* d_perm, void* d_tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_loki_groups(uint64_t n, const LokiPlanDev& D, const uint64_t* d_key_sorted, const uint32_t* d_perm, uint32_t* d_flag,
                              uint32_t* d_gidx, uint32_t* d_esz, uint64_t* d_E, uint32_t* d_gs, nfagg_loki_group* d_groups, void* d_tmp,
                              size_t tmp_bytes, const LokiScan& X, hipStream_t s);
size_t loki_tmp_bytes(uint64_t n);
// write
struct LokiWriteDev {
    const LokiCtl* ctl;
    const uint32_t* perm; const uint32_t* flag; const uint32_t* gidx; const uint64_t* E; const uint32_t* gs;
    const nfagg_loki_group* groups;
    const uint8_t* labels; const uint32_t* lab_off;      // the streams' label text, n_streams + 1 offsets
    uint32_t* hsz; uint64_t* H;                          // per group: the header's size; their exclusive scan (n_groups + 1)
    uint32_t* local_off; uint64_t* block_base;           // the positions' offsets in the skeleton's two-level form
    uint32_t* bpos;                                      // per batch: its first position (n_batches + 1)
};
hipError_t launch_loki_offsets(uint32_t m, uint32_t n_groups, uint32_t n_batches, const LokiWriteDev& W, uint64_t* d_batch_offsets,
                               uint32_t* d_batch_entries, const LokiScan& X, hipStream_t s);
hipError_t launch_loki_write(const FlpLineArgs& A, bool content, const LokiDev& L, const LokiPlanDev& D, const LokiWriteDev& W, uint32_t m, uint32_t n_groups,
                             uint8_t* d_out, hipStream_t s);
uint32_t loki_max_entry(int policy);
// nfagg_flp_content.hip: the same two kernels over FlpContent and FlpContentNetev (A.F.ne_rows selects)
hipError_t launch_loki_key_content(const FlpLineArgs& A, const LokiDev& L, const LokiPlanDev& D, hipStream_t s);
hipError_t launch_loki_write_content(const FlpLineArgs& A, const LokiDev& L, const LokiPlanDev& D, const LokiWriteDev& W, uint32_t m, uint8_t* d_out, hipStream_t s);
uint32_t loki_max_entry_content(int policy);

}  // namespace nfagg
