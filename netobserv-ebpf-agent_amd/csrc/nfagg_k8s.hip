// nfagg_k8s.hip — the hash join of a flow's two addresses against the Kubernetes table (nfagg_k8s.h), one lane per flow:
// what datasource.IndexLookup(nil, ip) is asked for SrcAddr and for DstAddr (enrich.go:38-47). A record whose
// eth_protocol is neither 0x0800 nor 0x86DD has no address key (LookupString fails) and gets no row, whatever its id
// bytes hold. A lane reads its record's 32 address bytes and the ethertype, not the whole record; a probe step is one
// aligned 32-byte slot.
#include "nfagg_k8s.h"

namespace nfagg {

constexpr int kK8sBlock = 256;

__global__ __launch_bounds__(kK8sBlock) void k_k8s_resolve(const void* __restrict__ recs, uint64_t n, K8sDev K, uint32_t* __restrict__ rows_out) {
    const uint64_t i = (uint64_t)blockIdx.x * kK8sBlock + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = reinterpret_cast<const uint8_t*>(recs) + i * kRecordBytes;
    const uint32_t eth = reinterpret_cast<const uint32_t*>(p)[17] & 0xffffu;       // Rec::eth()
    uint32_t src = kK8sNoRow, dst = kK8sNoRow;
    if (eth == 0x0800u || eth == 0x86DDu) {
        const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
        src = k8s_probe(K, a.x, a.y, a.z, a.w);
        dst = k8s_probe(K, b.x, b.y, b.z, b.w);
    }
    reinterpret_cast<uint2*>(rows_out)[i] = make_uint2(src, dst);
}

hipError_t launch_k8s_resolve(const void* d_recs, uint64_t n, const K8sDev& K, uint32_t* d_rows_out, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_k8s_resolve, dim3((unsigned)((n + kK8sBlock - 1) / kK8sBlock)), dim3(kK8sBlock), 0, s, d_recs, n, K, d_rows_out);
    return hipGetLastError();
}

}  // namespace nfagg
