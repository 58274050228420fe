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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nfagg_flp.h"

namespace nfagg {

constexpr uint32_t kMetMaxGroupings = NFAGG_MET_MAX_GROUPINGS, kMetMaxGroups = NFAGG_MET_MAX_GROUPS;
constexpr uint32_t kMetSlotWords = 8, kMetMinSlots = 1024;          // kMetMinSlots = kScanBlock: a block of k_metrics_count lies in one grouping
constexpr uint32_t kMetSrcFields = 0x1ffu, kMetDstFields = 0x1ffu << 9;
constexpr uint64_t kMetMark = 1ull << 63;
static_assert(sizeof(nfagg_metric_group) == 64 && kMetSlotWords * 8 == 64, "nfagg_metric_group layout");
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
    nfagg_metric_group* out[kMetMaxGroupings];
    uint32_t mask[kMetMaxGroupings], cap[kMetMaxGroupings], dims[kMetMaxGroupings];
    uint32_t first_block[kMetMaxGroupings + 1];   // k_metrics_count / k_metrics_emit: grouping g's slots are blocks [first_block[g], first_block[g + 1])
    MetCtl* ctl;
    const K8sRow* rows;                      // the app flags, read when a grouping selects the layer
    uint32_t n_groupings, n_rows, has_layer, any_layer;
};

// d_net_rows may be nullptr when no grouping selects a label or the direction. The caller has zeroed ctl and the slots on s.
hipError_t launch_metrics_fold(const void* d_recs, uint64_t n, const MetDev& M, const uint32_t* d_k8s_rows, const uint2* d_net_rows, hipStream_t s);
// Count the occupied slots (local_off, block_sum: one word per slot, per block), scan the block sums (block_base: blocks + 1
// words), then write ctl->count / ctl->over and, only if no grouping is over, the groups.
hipError_t launch_metrics_emit(const MetDev& M, uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s);

}  // namespace nfagg
