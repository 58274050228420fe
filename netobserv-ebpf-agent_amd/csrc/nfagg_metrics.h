// nfagg_metrics.h — the GROUP BY under flowlogs-pipeline's `encode prom` counters (include/nfagg.h, "Flow metrics"): what the
// host hands the three kernels of nfagg_metrics.hip, and the layout of a group's key and slot. Host + device.
//
// Key: 16 bytes as two 64-bit halves. Bit 63 of each half is always set and each half carries the grouping's index, so the
// all-zero "empty" value is never a key and two groupings never share one:
//   A = 1<<63 | g<<58 | dst_class<<29 | src_class          (a class is at most NFAGG_K8S_MAX_ROWS = 2^22)
//   B = 1<<63 | g<<56 | is_ip<<50 | proto<<42 | layer<<40 | direction<<32 | dst_label<<16 | src_label
// Slot of a grouping's global table: eight 64-bit words {A, B, flows, bytes, packets, flows_with_bytes, flows_with_packets,
// 0}; a table is a power of two of slots, at least kMetMinSlots and at least twice the caller's cap, probed linearly from the
// low bits of met_hash(A, B).
//
// The content fold (nfagg_metrics_fold_content: histograms, the values and labels of the feature parts) has a third key word
//   C = 1<<63 | g<<56 | bucket6<<48 | ipsec<<46 | rcode5<<41 | state9<<32 | drop_cause
// with the public "none" values masked to the field's width (bucket 0xFF -> 63, rcode 0xFF -> 31, state 0xFFFF -> 511; a real
// bucket is at most 32, a real code at most 15, a real state at most 255), and sixteen words per slot: {A, B, C, 0, flows, bytes,
// packets, flows_with_bytes, flows_with_packets, value_sum[2], flows_with_value[2], 0, 0, 0}, so that words 4..15 are bytes
// 32..127 of nfagg_metric_group_content as they stand. Probed from the low bits of met_hash(A, B, C).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "nfagg_flp.h"

namespace nfagg {

constexpr uint32_t kMetMaxGroupings = NFAGG_MET_MAX_GROUPINGS, kMetMaxGroups = NFAGG_MET_MAX_GROUPS;
constexpr uint32_t kMetSlotWords = 8, kMetcSlotWords = 16, kMetMinSlots = 1024;          // kMetMinSlots = kScanBlock: a block of k_metrics_count lies in one grouping
constexpr uint32_t kMetSrcFields = 0x1ffu, kMetDstFields = 0x1ffu << 9;
constexpr uint64_t kMetMark = 1ull << 63;
static_assert(sizeof(nfagg_metric_group) == 64 && kMetSlotWords * 8 == 64, "nfagg_metric_group layout");
static_assert(sizeof(nfagg_metric_group_content) == 128 && kMetcSlotWords * 8 == 128 && offsetof(nfagg_metric_group_content, flows) == 32 &&
              offsetof(nfagg_metric_group_content, value_sum) == 72 && offsetof(nfagg_metric_group_content, bucket) == 24, "nfagg_metric_group_content layout");
static_assert(sizeof(nfagg_metric_spec) == 24 + 8 * NFAGG_MET_MAX_BOUNDS && NFAGG_MET_MAX_BOUNDS < 63, "nfagg_metric_spec layout, the key's bucket field");
static_assert(NFAGG_K8S_MAX_ROWS < (1u << 29) && kMetMaxGroupings <= 8, "the key's class and grouping fields");

NF_HD uint64_t met_key_a(uint32_t g, uint32_t src_class, uint32_t dst_class) {
    return kMetMark | ((uint64_t)g << 58) | ((uint64_t)dst_class << 29) | (uint64_t)src_class;
}
NF_HD uint64_t met_key_b(uint32_t g, uint32_t src_label, uint32_t dst_label, uint32_t direction, uint32_t layer, uint32_t proto, uint32_t is_ip) {
    return kMetMark | ((uint64_t)g << 56) | ((uint64_t)is_ip << 50) | ((uint64_t)proto << 42) | ((uint64_t)layer << 40) | ((uint64_t)direction << 32) |
           ((uint64_t)dst_label << 16) | (uint64_t)src_label;
}
NF_HD uint32_t met_key_grouping(uint64_t a) { return (uint32_t)(a >> 58) & 7u; }
NF_HD uint64_t met_hash(uint64_t a, uint64_t b) { return fmix64((rotl64(a * kMul, 27) ^ b) * kMul); }
NF_HD uint64_t met_key_c(uint32_t g, uint32_t drop_cause, uint32_t drop_state, uint32_t dns_rcode, uint32_t ipsec_status, uint32_t bucket) {
    return kMetMark | ((uint64_t)g << 56) | ((uint64_t)(bucket & 0x3fu) << 48) | ((uint64_t)(ipsec_status & 3u) << 46) | ((uint64_t)(dns_rcode & 0x1fu) << 41) |
           ((uint64_t)(drop_state & 0x1ffu) << 32) | (uint64_t)drop_cause;
}
NF_HD uint64_t met_hash(uint64_t a, uint64_t b, uint64_t c) { return fmix64((rotl64(met_hash(a, b), 27) ^ c) * kMul); }

// Control words at the head of the slot scratch, zeroed with it by the call's one memset; the last 16 are the call's one read-back.
struct MetCtl {
    uint32_t claimed[kMetMaxGroupings];      // slots claimed in grouping g's table = its distinct groups so far
    uint32_t overflow[kMetMaxGroupings];     // grouping g has more groups than its cap (claimed > cap, or its table is full)
    uint32_t count[kMetMaxGroupings];        // k_metrics_emit: occupied slots of grouping g
    uint32_t over[kMetMaxGroupings];         // k_metrics_emit: overflow[g] || count[g] > cap[g]
};
static_assert(sizeof(MetCtl) == 128, "MetCtl layout");

struct MetDev {
    uint64_t* slots[kMetMaxGroupings];       // grouping g's table: (mask[g] + 1) slots of kMetSlotWords words
    const uint32_t* cls[kMetMaxGroupings][2];   // the rows' classes, per side; nullptr: the grouping selects no field of that side
    void* out[kMetMaxGroupings];             // nfagg_metric_group[cap], or nfagg_metric_group_content[cap] in the content fold
    uint32_t mask[kMetMaxGroupings], cap[kMetMaxGroupings], dims[kMetMaxGroupings];
    uint32_t first_block[kMetMaxGroupings + 1];   // k_metrics_count / k_metrics_emit: grouping g's slots are blocks [first_block[g], first_block[g + 1])
    MetCtl* ctl;
    const K8sRow* rows;                      // the app flags, read when a grouping selects the layer
    uint32_t n_groupings, n_rows, has_layer, any_layer;
};

// What the content fold adds to MetDev: the specs, and which parts some grouping needs (uniform per call, so a lane's loads
// branch on scalars). The bounds ride in the kernel arguments: 2 KiB read with scalar loads, at uniform indexes only.
constexpr uint32_t kMetNeedAdditional = 1, kMetNeedDns = 2, kMetNeedDrops = 4;
struct MetSpecDev {
    int64_t bounds[kMetMaxGroupings][NFAGG_MET_MAX_BOUNDS];
    uint32_t xdims[kMetMaxGroupings];
    uint8_t value[kMetMaxGroupings][2];
    uint8_t hist[kMetMaxGroupings], n_bounds[kMetMaxGroupings];
    uint32_t need;                           // kMetNeed*: parts that a value source or an extra dimension of some grouping reads AND whose array was given
    const uint8_t* present;                  // the flows' NFAGG_FEAT_* bytes, or nullptr
    const uint8_t* additional;               // nfagg_additional_metrics[n]
    const uint8_t* dns;                      // nfagg_dns_metrics[n]
    const uint8_t* drops;                    // nfagg_pkt_drop_metrics[n]
};

// d_net_rows may be nullptr when no grouping selects a label or the direction. The caller has zeroed ctl and the slots on s.
hipError_t launch_metrics_fold(const void* d_recs, uint64_t n, const MetDev& M, const uint32_t* d_k8s_rows, const uint2* d_net_rows, hipStream_t s);
// Count the occupied slots (local_off, block_sum: one word per slot, per block), scan the block sums (block_base: blocks + 1
// words), then write ctl->count / ctl->over and, only if no grouping is over, the groups.
// content: the tables have kMetcSlotWords per slot and the groups are nfagg_metric_group_content.
hipError_t launch_metrics_emit(const MetDev& M, bool content, uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s);
// The content fold: as launch_metrics_fold over slots of kMetcSlotWords.
hipError_t launch_metrics_fold_content(const void* d_recs, uint64_t n, const MetDev& M, const MetSpecDev& X, const uint32_t* d_k8s_rows, const uint2* d_net_rows,
                                       hipStream_t s);

}  // namespace nfagg
