// nfagg_conn_json.h — extract conntrack's conversation records as JSON lines (nfagg_conn_json.hip): the column program a
// layout compiles to, as the host builds it and the kernels walk it, and the two launches.
#pragma once
#include "nfagg_flp.h"

namespace nfagg {

// One column of a line, in sorted order. frag: ,"name": in the layout's blob, at a 16-byte aligned offset (no fragment for a block).
enum : uint32_t { kConnColKey = 0, kConnColBlock = 1, kConnColMeta = 2, kConnColAgg = 3, kConnColSnap = 4 };
//   key    arg: 0 SrcAddr, 1 DstAddr, 2 SrcPort, 3 DstPort, 4 Proto                         from the carrier
//   block  arg: 0 DstK8S_*, 1 DstSubnetLabel, 2 K8S_FlowLayer, 3 SrcK8S_*, 4 SrcSubnetLabel   from the carrier's rows
//   meta   arg: 0 _HashId, 1 _IsFirst, 2 _RecordType
//   agg    arg: source (0 flows, 1 bytes, 2 packets, 3 start_ms_min, 4 end_ms_max) | side << 8 (0 both, 1 AB, 2 BA); omitted when 0
//   snap   arg: NFAGG_CONN_IN_* | which << 8 (0 first, 1 last)
struct ConnCol { uint32_t kind, arg, frag_off, frag_len; };
static_assert(sizeof(ConnCol) == 16, "column program");
struct ConnLayoutDev { const ConnCol* cols; const uint8_t* blob; uint32_t n_cols; };

// The longest line a layout may reach: what leaves the write kernel a window of 16 384 in 32 KiB beside 16 bytes of side LDS.
constexpr uint32_t kConnLineCap = 32768 - 16 - 16384;
static_assert(kConnLineCap % 16 == 0, "the window's LDS");
// The longest value of each column kind, for the layout's own bound (host side).
constexpr uint32_t kConnAddrMax = 2 + 39, kConnMacMax = 2 + 17, kConnAggMax = 17, kConnI64Max = 20, kConnDirsMax = 2 + 7 * 3 + 6,
                   kConnHashIdMax = 2 + 16, kConnIsFirstMax = 5, kConnRecordTypeMax = 2 + 13;

// d_lens: one dword per conversation, size pass -> write pass (0: deferred). d_n_deferred: zeroed by the caller.
hipError_t launch_conn_json_size(const void* d_carriers, const void* d_values, uint64_t n, const ConnLayoutDev& L, const K8sDev& K, const NetDev& N,
                                 const uint32_t* d_k8s_rows, const uint2* d_net_rows, uint32_t* d_lens, uint32_t* d_local_off, uint32_t* d_block_sum,
                                 uint64_t* d_block_base, uint32_t* d_n_deferred, hipStream_t s);
hipError_t launch_conn_json_write(const void* d_carriers, const void* d_values, uint64_t n, const ConnLayoutDev& L, const K8sDev& K, const NetDev& N,
                                  const uint32_t* d_k8s_rows, const uint2* d_net_rows, const uint32_t* d_lens, const uint32_t* d_local_off,
                                  const uint64_t* d_block_base, void* d_out, uint64_t* d_line_offsets, uint8_t* d_deferred, hipStream_t s);

}  // namespace nfagg
