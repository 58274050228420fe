// nfagg_net.hip — the join of nfagg_net_resolve, one lane per flow (nfagg_net.h): the first-match walk of the CIDR list that
// applySubnetLabel does for SrcAddr and for DstAddr (transform_network.go:185-196), and reinterpretDirection's three string
// compares (transform_network_direction.go:52-63) as compares of interned ids. A lane reads its record's ethertype dword
// and 32 address bytes, its two Kubernetes rows and their host ids, and stores 8 bytes. The walk reads entry k for the whole
// wave at once: the index is uniform, so the entry arrives through the scalar cache, 32 + 4 bytes per step for 64 flows; a
// lane drops out when both its addresses have their answer, the wave when its last lane has.
#include "nfagg_net.h"

namespace nfagg {

constexpr int kNetBlock = 256;

__global__ __launch_bounds__(kNetBlock) void k_net_resolve(const void* __restrict__ recs, uint64_t n, NetDev N, const uint32_t* __restrict__ k8s_rows,
                                                           const uint32_t* __restrict__ host_ids, uint32_t n_k8s_rows, uint32_t reporter,
                                                           uint2* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kNetBlock + threadIdx.x;
    if (i >= n) return;
    uint32_t label[2] = {kNetNoLabel, kNetNoLabel};
    if (N.flags & NFAGG_NET_SUBNET_LABELS) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(recs) + i * kRecordBytes;
        const uint32_t eth = reinterpret_cast<const uint32_t*>(p)[17] & 0xffffu;   // Rec::eth()
        if (eth == 0x0800u || eth == 0x86DDu) {                                    // else: no SrcAddr / DstAddr key, no label
            const uint4 a[2] = {reinterpret_cast<const uint4*>(p)[0], reinterpret_cast<const uint4*>(p)[1]};
            const bool v4[2] = {(a[0].x | a[0].y) == 0 && a[0].z == 0xffff0000u, (a[1].x | a[1].y) == 0 && a[1].z == 0xffff0000u};
            bool open[2] = {true, true};
            for (uint32_t k = 0; k < N.n_cidrs && (open[0] || open[1]); k++) {
                const NetCidr c = N.cidrs[k];
                const uint32_t meta = N.meta[k];
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const bool hit = (a[e].x & c.mask[0]) == c.net[0] && (a[e].y & c.mask[1]) == c.net[1] && (a[e].z & c.mask[2]) == c.net[2] &&
                                     (a[e].w & c.mask[3]) == c.net[3] && !((meta & kNetCidrV6) && v4[e]);
                    if (open[e] && hit) { label[e] = meta & 0xffffu; open[e] = false; }
                }
            }
        }
    }
    uint32_t dir = kNetNoDirection;
    if (N.flags & NFAGG_NET_REINTERPRET_DIRECTION) {
        const uint2 rows = reinterpret_cast<const uint2*>(k8s_rows)[i];
        const uint32_t s = rows.x < n_k8s_rows ? host_ids[rows.x] : 0u, d = rows.y < n_k8s_rows ? host_ids[rows.y] : 0u;   // 0: the key is absent, ""
        if (s != d) dir = s == reporter ? 1u : d == reporter ? 0u : kNetNoDirection;      // egress, ingress
        else if (s != 0) dir = 2u;                                                        // inner
    }
    out[i] = make_uint2(label[0] | (label[1] << 16), dir);
}

hipError_t launch_net_resolve(const void* d_recs, uint64_t n, const NetDev& N, const uint32_t* d_k8s_rows, const uint32_t* d_host_ids,
                              uint32_t n_k8s_rows, uint32_t reporter, uint2* d_out, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_net_resolve, dim3((unsigned)((n + kNetBlock - 1) / kNetBlock)), dim3(kNetBlock), 0, s, d_recs, n, N, d_k8s_rows, d_host_ids,
                       n_k8s_rows, reporter, d_out);
    return hipGetLastError();
}

}  // namespace nfagg
