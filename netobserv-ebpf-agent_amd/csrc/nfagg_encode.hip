// nfagg_encode.hip — the middle kernel of every two-pass job (the export encoders, the rollup, the map merge): exclusive
// scan of the block sums a size kernel left (one workgroup), total in block_base[n_blocks].
#include "nfagg_encode.h"

namespace nfagg {

__global__ __launch_bounds__(1024) void k_scan_block_sums(const uint32_t* __restrict__ block_sum, uint32_t n_blocks,
                                                          uint64_t* __restrict__ block_base) {
    __shared__ uint64_t part[1024];
    const uint32_t per = (n_blocks + 1023) / 1024;
    const uint32_t lo = threadIdx.x * per, hi = (lo + per < n_blocks) ? lo + per : n_blocks;
    uint64_t s = 0;
    for (uint32_t k = lo; k < hi; k++) s += block_sum[k];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { uint64_t acc = 0; for (int k = 0; k < 1024; k++) { const uint64_t x = part[k]; part[k] = acc; acc += x; } block_base[n_blocks] = acc; }
    __syncthreads();
    uint64_t acc = part[threadIdx.x];
    for (uint32_t k = lo; k < hi; k++) { block_base[k] = acc; acc += block_sum[k]; }
}

hipError_t launch_scan_block_sums(const uint32_t* d_block_sum, uint32_t n_blocks, uint64_t* d_block_base, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(1024), 0, s, d_block_sum, n_blocks, d_block_base);
    return hipGetLastError();
}

}  // namespace nfagg
