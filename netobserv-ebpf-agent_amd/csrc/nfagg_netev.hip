// nfagg_netev.hip — network events of MapTracer flows against the cookie table: the loop of
//   pkg/model/record.go:126-157          NewRecord with a SampleDecoder
//   pkg/utils/networkevents/network_events.go:121-131   ToDropReasonCode (as the table's `cause` column)
//   pkg/model/flow_content.go:209-215    addUint16
// one lane per flow. The decoder's answers arrive as the sorted table of nfagg_netev.h; a cookie without a row goes
// into the caller's open-addressed set (64-bit compare-and-swap), so the host learns what to ask its decoder next
// without walking the flows.
#include "nfagg_encode.h"
#include "nfagg_netev.h"

namespace nfagg {

constexpr int kNetevBlock = 256;
constexpr uint32_t kNetevLdsRows = 256;      // a table of up to this many rows is searched in LDS (16 B per row: 4 KiB)

// Row of `cookie` in the sorted table, kNetevNoRow when there is none. `base`: the rows' first 16 bytes, STRIDE apart.
template <uint32_t STRIDE> NF_DEV uint32_t netev_find(const uint8_t* base, uint32_t n_rows, uint64_t cookie) {
    uint32_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (*reinterpret_cast<const uint64_t*>(base + (size_t)mid * STRIDE) < cookie) lo = mid + 1; else hi = mid;
    }
    return lo < n_rows && *reinterpret_cast<const uint64_t*>(base + (size_t)lo * STRIDE) == cookie ? lo : kNetevNoRow;
}

NF_DEV uint64_t netev_mix(uint64_t x) {      // splitmix64's finalizer
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31;
    return x;
}

// info: [0] distinct cookies recorded, [1] overflow, [2] the all-zero cookie (which a slot cannot hold) was missing
NF_DEV void netev_missing(unsigned long long* set, uint32_t cap, uint32_t* info, uint64_t cookie) {
    if (cookie == 0) { if (atomicExch(&info[2], 1u) == 0u) atomicAdd(&info[0], 1u); return; }
    uint32_t s = cap ? (uint32_t)(netev_mix(cookie) % cap) : 0u;
    for (uint32_t t = 0; t < cap; t++) {
        unsigned long long old = __hip_atomic_load(&set[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0ull) old = atomicCAS(&set[s], 0ull, (unsigned long long)cookie);
        if (old == 0ull) { atomicAdd(&info[0], 1u); return; }
        if (old == cookie) return;
        s = s + 1 == cap ? 0u : s + 1;
    }
    atomicOr(&info[1], 1u);
}

NF_DEV uint32_t sat16(uint32_t a, uint32_t b) { const uint32_t v = a + b; return v > 0xffffu ? 0xffffu : v; }

__global__ __launch_bounds__(kNetevBlock) void k_netev_resolve(const uint8_t* present, const uint8_t* netev, const uint8_t* drops, uint64_t n,
                                                               const NetevRow* __restrict__ rows, uint32_t n_rows, uint8_t* present_out,
                                                               uint8_t* drops_out, uint16_t* rows_out, unsigned long long* missing_set,
                                                               uint32_t missing_cap, uint32_t* missing_info) {
    __shared__ uint4 tab_lds[kNetevLdsRows];
    const bool staged = n_rows <= kNetevLdsRows;
    if (staged) {
        for (uint32_t k = threadIdx.x; k < n_rows; k += kNetevBlock) tab_lds[k] = reinterpret_cast<const uint4*>(rows)[2 * k];
        __syncthreads();
    }
    const uint64_t i = (uint64_t)blockIdx.x * kNetevBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = present[i];
    bool have_drops = drops && (p & NFAGG_FEAT_DROPS);
    uint32_t dw[8] = {};                   // pkt_drop_metrics: start@0 end@8 bytes@16 packets@18 cause@20 flags@24 eth@26 state@28
    if (have_drops) load_dwords8(drops + i * 32, dw);
    uint32_t ev[4] = {kNetevNoRow, kNetevNoRow, kNetevNoRow, kNetevNoRow}, cls[4] = {};
    uint32_t cnt = 0;
    if (netev && (p & NFAGG_FEAT_NETWORK_EVENTS)) {
        uint32_t w[18];                    // network_events_metrics: start@0 end@8 cookies@16 bytes@48 packets@56
        load_dwords8(netev + i * 72, w);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t pk = (w[14 + (k >> 1)] >> (16 * (k & 1))) & 0xffffu, by = (w[12 + (k >> 1)] >> (16 * (k & 1))) & 0xffffu;
            if (pk == 0) continue;
            const uint64_t cookie = (uint64_t)w[4 + 2 * k] | ((uint64_t)w[5 + 2 * k] << 32);
            const uint32_t r = staged ? netev_find<16>(reinterpret_cast<const uint8_t*>(tab_lds), n_rows, cookie)
                                      : netev_find<32>(reinterpret_cast<const uint8_t*>(rows), n_rows, cookie);
            if (r == kNetevNoRow) { netev_missing(missing_set, missing_cap, missing_info, cookie); continue; }
            const uint4 m = staged ? tab_lds[r] : reinterpret_cast<const uint4*>(rows)[2 * r];
            const uint32_t c = m.z & 0xffffu, kind = m.z >> 16, cause = m.w;
            if (kind == NFAGG_NETEV_UNDECODABLE) continue;
            bool seen = false;
#pragma unroll
            for (int j = 0; j < 4; j++) seen = seen || ((uint32_t)j < cnt && cls[j] == c);
            if (!seen) {
#pragma unroll
                for (int j = 0; j < 4; j++) if ((uint32_t)j == cnt) { ev[j] = r; cls[j] = c; }
                cnt++;
            }
            if (cause) {
                if (!have_drops) {
                    dw[0] = w[0]; dw[1] = w[1]; dw[2] = w[2]; dw[3] = w[3];
                    dw[4] = by | (pk << 16); dw[5] = cause; dw[6] = 0; dw[7] = 0;
                    have_drops = true;
                } else {
                    dw[4] = sat16(dw[4] & 0xffffu, by) | (sat16(dw[4] >> 16, pk) << 16);
                    dw[5] = cause;
                }
            }
        }
    }
    if (!have_drops) {
#pragma unroll
        for (int k = 0; k < 8; k++) dw[k] = 0;
    }
    present_out[i] = (uint8_t)((p & ~(uint32_t)NFAGG_FEAT_DROPS) | (have_drops ? (uint32_t)NFAGG_FEAT_DROPS : 0u));
    uint2* d = reinterpret_cast<uint2*>(drops_out + i * 32);
#pragma unroll
    for (int k = 0; k < 4; k++) d[k] = make_uint2(dw[2 * k], dw[2 * k + 1]);
    reinterpret_cast<uint2*>(rows_out)[i] = make_uint2(ev[0] | (ev[1] << 16), ev[2] | (ev[3] << 16));
}

hipError_t launch_netev_resolve(const uint8_t* d_present, const uint8_t* d_netev, const uint8_t* d_drops, uint64_t n,
                                const NetevRow* d_rows, uint32_t n_rows, uint8_t* d_present_out, uint8_t* d_drops_out,
                                uint16_t* d_rows_out, uint64_t* d_missing_set, uint32_t missing_cap, uint32_t* d_missing_info,
                                hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_netev_resolve, dim3((unsigned)((n + kNetevBlock - 1) / kNetevBlock)), dim3(kNetevBlock), 0, s, d_present, d_netev,
                       d_drops, n, d_rows, n_rows, d_present_out, d_drops_out, d_rows_out, (unsigned long long*)d_missing_set, missing_cap,
                       d_missing_info);
    return hipGetLastError();
}

}  // namespace nfagg
