// nfagg_filter.h — flowlogs-pipeline's `transform filter` stage as a device program (include/nfagg.h, "transform filter";
// DESIGN.md §4.7o): the compiled form the kernels of nfagg_filter.hip read, the counter-based roll, and the launchers.
// A filter is atoms (predicates over the small integers a flow already is on the device), a postfix stream of atom indexes
// and AND / OR / NOT, and steps that each own a slice of the stream. The program is the same for every lane, so the
// interpreter loop is wave-uniform; its evaluation stack is one 64-bit mask per lane, one bit per level.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nfagg.h"
#include "nfagg_flp.h"
#include "nfagg_hash.h"
#include "nfagg_pb.h"

namespace nfagg {

constexpr uint32_t kFilterMaxAtoms = NFAGG_FILTER_MAX_ATOMS, kFilterMaxOps = NFAGG_FILTER_MAX_OPS, kFilterMaxSteps = NFAGG_FILTER_MAX_STEPS;
constexpr uint32_t kFilterMaxStack = NFAGG_FILTER_MAX_STACK;
constexpr uint32_t kFilterScanBlock = 1024;   // kScanBlock (nfagg_encode.h), for the host side's scratch sizes

// What a program reads beside the record: the kernel loads only what `need` names.
constexpr uint32_t kFilterNeedK8s = 1u, kFilterNeedNet = 2u, kFilterNeedAdditional = 4u, kFilterNeedDns = 8u, kFilterNeedDrops = 16u,
                   kFilterNeedClock = 32u, kFilterNeedK8sRow = 64u;   // NeedK8sRow: the rows' app flags (flow layer)
// Program flags
constexpr uint32_t kFilterStore = 1u;        // samplingField == "Sampling": the admitting keep rule multiplies
constexpr uint32_t kFilterFlagNames = 2u;    // NFAGG_NET_DECODE_TCP_FLAGS: Flags is a []string, no number

struct FilterAtom {            // 48 bytes
    uint32_t kind;             // NFAGG_FILTER_ATOM_*
    uint32_t a;                // NUM / PRESENT: the field; TABLE: the dimension; ADDR / MAC: the side; CONST: the value
    uint32_t cmp;              // NUM: NFAGG_FILTER_CMP_*
    uint32_t n_truth;          // TABLE: entries, the last one for "none"
    int64_t value;             // NUM
    uint64_t truth_off;        // TABLE: first byte in the truth blob
    uint32_t w[4];             // ADDR: the 16 bytes as four little-endian dwords; MAC: the 6 bytes, byte 0 in the low bits of w[0]
};
struct FilterStep { uint32_t kind, group, value, op_begin, op_count, pad_[3]; };   // 32 bytes
struct FilterProg {
    uint32_t n_atoms, n_ops, n_steps, n_keep;    // n_keep: the KEEP steps, which come first
    uint32_t flags, need, pad_[2];
    FilterStep steps[kFilterMaxSteps];
    FilterAtom atoms[kFilterMaxAtoms];
    uint8_t ops[kFilterMaxOps];
};
static_assert(sizeof(FilterAtom) == 48 && sizeof(FilterStep) == 32 && sizeof(FilterProg) % 16 == 0, "filter program layout");

// The call's clocks, as FlpParams carries them (record.go:90-97).
struct FilterClock { int64_t now_sec, now_nsec; uint64_t mono_now; };

// The roll of step `step` for the flow with running index `flow_index`: a function of (seed, flow_index, step) alone, so a
// call split in two, or repeated, rolls the same. The flow is sampled in iff u % value == 0 (value 0: always).
NF_HD uint64_t filter_roll_u(uint64_t seed, uint64_t flow_index, uint32_t step) {
    return fmix64(fmix64(seed + kMul * flow_index) ^ (kMul * ((uint64_t)step + 1)));
}
NF_HD bool filter_roll(uint64_t seed, uint64_t flow_index, uint32_t step, uint32_t value) {
    return value == 0 || filter_roll_u(seed, flow_index, step) % value == 0;
}

// k_filter_eval, the scan of the block sums, nothing else: keep / rule / samp per flow, local_off and block_base such that flow
// i's place among the kept is block_base[i / 1024] + local_off[i]; block_base[blocks] = the kept; *d_n_deferred += the deferred.
hipError_t launch_filter_eval(const void* d_recs, uint64_t n, const FilterProg* d_prog, const uint8_t* d_truth, const PbFeat& F,
                              const uint32_t* d_k8s_rows, const K8sDev& K, const uint2* d_net_rows, const FilterClock& clk, uint64_t seed,
                              uint64_t first_index, uint8_t* d_keep, uint8_t* d_rule, uint32_t* d_samp, uint32_t* d_local_off,
                              uint32_t* d_block_sum, uint64_t* d_block_base, uint32_t* d_n_deferred, hipStream_t s);
// k_filter_compact: kept_idx, and (d_out != nullptr) the kept records with their sampling rewritten.
hipError_t launch_filter_compact(const void* d_recs, uint64_t n, const uint32_t* d_samp, const uint32_t* d_local_off,
                                 const uint64_t* d_block_base, uint32_t* d_kept_idx, void* d_out, hipStream_t s);
// k_gather: dst[j] = src[idx[j]] in units of `unit` bytes (1, 2, 4, 8 or 16; elem_bytes a multiple of it); an index from
// n_src up yields zeros.
hipError_t launch_gather(const void* d_src, uint64_t n_src, uint32_t elem_bytes, uint32_t unit, const uint32_t* d_idx, uint64_t n_kept, void* d_dst,
                         hipStream_t s);

}  // namespace nfagg
