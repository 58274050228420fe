// nfagg_flp_ipfix.h — launch interface of write ipfix on the device (nfagg_flp_ipfix.hip; include/nfagg.h, "write ipfix on the
// device"): the strings table's rows, the carry groups, the per-call arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nfagg.h"
#include "nfagg_pb.h"

namespace nfagg {

// A carry group: the elements one conditionally absent key of the flow's map feeds (write_ipfix.go:526-537 with
// decode_protobuf.go:87-182). Group g of flow i is set when the key exists; otherwise the elements keep what the last flow
// of the same family with the group set left, or the writer's state.
enum : uint32_t {
    kIxBytes = 0, kIxPackets, kIxSampling, kIxAddr, kIxIcmp, kIxPorts, kIxFlags, kIxXlatSrcPort, kIxXlatDstPort, kIxRtt,
    kIxStr0,                        // six Kubernetes strings: SrcNamespace SrcName DstNamespace DstName SrcHostName DstHostName
    kIxGroups = kIxStr0 + 6,        // 16 groups a flow keeps a source for
    kIxAny = kIxGroups,             // "a flow of this family": what the state export takes the always-set elements from
    kIxAggs = kIxAny + 1            // 17 aggregates per family
};
constexpr int32_t kIxFromState = -1;      // source: the writer's state
constexpr int32_t kIxOpen = -2;           // k_ipfix_carry: no source in the flow's block; k_ipfix_size closes it
constexpr uint32_t kIxMetaV6 = 1u << 31;  // meta[i]: the group bits, the family on top, the status (from k_ipfix_flp_size on)
constexpr uint32_t kIxMetaStatusShift = 24;
constexpr uint32_t kIxScanThreads = 64;   // k_ipfix_carry_scan: a call of 2^16 flows already gives every thread more than one block

// One row of the strings table: namespace, name, host name of entries[r]. off: byte offset of the text in the blob, 16-byte
// aligned; len: its bytes; present: bit f = the key exists.
struct IxStrRow { uint32_t off[3]; uint32_t len[3]; uint32_t present; uint32_t pad_; };
static_assert(sizeof(IxStrRow) == 32, "strings row");

struct IxArgs {
    const void* recs; uint64_t n;
    PbFeat F;                              // present, additional (RTT) and xlat are read
    const uint32_t* k8s_rows;              // 2 x n, or null
    const IxStrRow* srows; const uint8_t* sblob; uint32_t n_srows;
    nfagg_flp_ipfix_elements* state;       // [2]: v4, v6
    const nfagg_intf_name* names; uint32_t n_names;
    uint32_t unknown_w[4]; uint32_t unknown_len;
    int64_t now_sec, now_nsec; uint64_t mono_now;
    uint32_t export_time, seq0, obs_domain, tid_v4, tid_v6, enterprise, max_msg, flags_mask;
    // scratch
    uint32_t* meta;                        // n
    int32_t* src;                          // n x kIxGroups
    int32_t* agg;                          // [2 * kIxAggs][blocks]: the last flow of the block with the group set, or -1
    int32_t* pre;                          // same shape: the last such flow before the block, or -1; [.][blocks] = after the last
    uint32_t* rows;                        // n x 8: seven interface rows and the message length (0: not sent)
    uint32_t* local_off; uint32_t* block_sum; uint64_t* block_base;      // bytes
    uint32_t* seq_local; uint32_t* seq_sum; uint64_t* seq_base;          // sent flows
};

hipError_t launch_ipfix_flp_plan(const IxArgs& A, hipStream_t s);      // presence, carry, size, the scans
hipError_t launch_ipfix_flp_write(const IxArgs& A, uint8_t* d_out, uint64_t* d_msg_offsets, uint8_t* d_status, hipStream_t s);   // write, state export

}  // namespace nfagg
