// nfagg_netev.h — the network-events cookie table as the kernels see it, and the launch interface of the resolve kernel
// (nfagg_netev.hip). The table is built and rendered on the host (nfagg_api_tables.hip, nfagg_netev_table_create).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nfagg.h"

namespace nfagg {

// One row, 32 bytes, rows sorted by `cookie` (the 8 cookie bytes as a little-endian value) for a binary search. The first
// 16 bytes are what the resolve kernel needs (and stages in LDS when the table is small), the second 16 what the
// encoders need. cls: the first row with the same String() bytes (kNetevNoRow: undecodable). cause: what
// networkevents.ToDropReasonCode gives, 0 = no drop. The rendered JSON object and pbflow.NetworkEvent of the row start
// at 16-byte aligned offsets of the blob and have at most NFAGG_NETEV_MAX_RENDERED bytes each.
struct NetevRow {
    uint64_t cookie;
    uint16_t cls, kind;
    uint32_t cause;
    uint32_t json_off, pb_off;
    uint16_t json_len, pb_len;
    uint32_t pad_;
};
static_assert(sizeof(NetevRow) == 32, "NetevRow layout");
constexpr uint32_t kNetevNoRow = NFAGG_NETEV_NO_ROW;
constexpr uint32_t kNetevMaxRendered = NFAGG_NETEV_MAX_RENDERED;

// The missing-cookie set's counters, four dwords of device memory: distinct cookies recorded, overflow flag, all-zero
// cookie seen, unused.
hipError_t launch_netev_resolve(const uint8_t* d_present, const uint8_t* d_netev, const uint8_t* d_drops, uint64_t n,
                                const NetevRow* d_rows, uint32_t n_rows, uint8_t* d_present_out, uint8_t* d_drops_out,
                                uint16_t* d_rows_out, uint64_t* d_missing_set, uint32_t missing_cap, uint32_t* d_missing_info,
                                hipStream_t s);

}  // namespace nfagg
