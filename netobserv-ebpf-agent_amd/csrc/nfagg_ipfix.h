// nfagg_ipfix.h — launch interface of the record -> IPFIX message kernels (nfagg_ipfix.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nfagg.h"

namespace nfagg {

struct IpfixParams {
    int64_t now_sec, now_nsec;    // currentTime, normalised (0 <= nsec < 1e9)
    uint64_t mono_now;
    const nfagg_intf_name* names; // device copy of the namer table, stably sorted by if_index
    uint32_t n_names;
    uint32_t unknown_len;
    uint32_t unknown_w[4];        // the unknown name's 16 bytes as little-endian dwords
    uint32_t export_time, seq0, obs_domain;
    uint32_t tid_v4, tid_v6;
};

// Message lengths (name row resolved once, kept in d_name_row: row + 1, 0 = unknown), block-local scan, scan of the
// block sums: d_block_base[ceil(n / 1024)] = total bytes afterwards.
hipError_t launch_ipfix_size(const void* d_recs, uint64_t n, const IpfixParams& P, uint32_t* d_name_row, uint32_t* d_local_off,
                             uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s);
hipError_t launch_ipfix_write(const void* d_recs, uint64_t n, const IpfixParams& P, const uint32_t* d_name_row, const uint32_t* d_local_off,
                              const uint64_t* d_block_base, void* d_out, uint64_t* d_msg_offsets, hipStream_t s);

}  // namespace nfagg
