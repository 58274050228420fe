// nfagg_metrics.hip — the hash aggregation of nfagg_metrics_fold (nfagg_metrics.h): k_metrics_fold groups the flows and sums,
// k_metrics_count / k_metrics_emit compact each grouping's occupied slots into the caller's arrays. Integer sums only, so the
// result does not depend on the order of the flows; no floating point anywhere.
//
// k_metrics_fold: grid-stride, one lane per flow, one workgroup per 4 096 flows up to 512 workgroups. A lane reads the three 16-byte units of its record that hold the protocol
// (@36), bytes (@56), packets (@64) and the ethertype (@68), its 8 bytes of Kubernetes rows and its 8 bytes of net row; per
// grouping the two class words, and K8sRow.flags of both rows once when a grouping selects the layer. Flows are pre-aggregated
// per workgroup in an LDS open-addressed table shared by the groupings (the key carries the grouping): kMetLdsSlots slots of
// key halves and five sums as seven arrays, 56 KiB, so that two workgroups fit a compute unit's 160 KiB. A lane whose probe of
// the LDS table passes kMetLdsProbe slots goes straight to the global table; at the end of the loop the workgroup flushes its
// LDS entries to the global tables.
//
// Claim protocol (LDS and global alike; nobody waits, no key is ever half published): compare-and-swap the first half from
// empty, go on if the old value was empty or equal to the lane's first half; then the second half likewise; a mismatch on
// either half moves to the next slot. A slot whose first half is set and whose second half is still empty can be taken by any
// key with that first half. Slots are never freed within a call and a set half never changes, so a key always ends in the
// same slot; whoever sets a first half goes on to the second, so at the end of the kernel no slot is half set.
//
// Overflow: a first half claimed from empty is one more occupied slot of that grouping, counted in MetCtl::claimed. A count
// over the cap, or a probe that has walked the whole table, sets MetCtl::overflow, and every later lane of that grouping gives
// up at once: the table has twice the cap's slots, so it does not fill up behind the flag except by the lanes already in
// flight, and a probe is bounded by the table's size whatever happens.
#include "nfagg_metrics.h"
#include "nfagg_encode.h"

namespace nfagg {

constexpr int kMetBlock = 512;
constexpr uint32_t kMetLdsSlots = 1024, kMetLdsProbe = 8, kMetMaxBlocks = 512;     // two workgroups per compute unit of 256
// A workgroup's flush costs up to kMetLdsSlots global claims and five adds each whatever it folded, so a workgroup is given
// at least this many flows: a call of a few hundred thousand flows then pays for tens of flushes, not for 512.
constexpr uint64_t kMetFlowsPerBlock = 4096;
static_assert(kMetLdsSlots * 7 * 8 * 2 <= 160 * 1024, "two workgroups' LDS tables in a compute unit");
static_assert(kMetMinSlots == kScanBlock, "a table is whole blocks of k_metrics_count");

struct MetLds {
    unsigned long long a[kMetLdsSlots], b[kMetLdsSlots], sum[5][kMetLdsSlots];
};

NF_DEV void met_global_add(const MetDev& M, uint32_t g, uint64_t ka, uint64_t kb, const uint64_t (&v)[5]) {
    uint32_t* over = &M.ctl->overflow[g];
    if (ald(over)) return;
    const uint32_t mask = M.mask[g];
    uint64_t* tab = M.slots[g];
    uint32_t s = (uint32_t)met_hash(ka, kb) & mask;
    for (uint32_t t = 0; t <= mask; t++) {
        uint64_t* p = tab + (size_t)s * kMetSlotWords;
        uint64_t a = ald(p);
        if (a == 0) {
            a = acas(p, (uint64_t)0, ka);
            if (a == 0 && aadd(&M.ctl->claimed[g], 1u) >= M.cap[g]) ast(over, 1u);      // this slot is number cap + 1 or later
        }
        if (a == 0 || a == ka) {
            uint64_t b = ald(p + 1);
            if (b == 0) b = acas(p + 1, (uint64_t)0, kb);
            if (b == 0 || b == kb) {
#pragma unroll
                for (int k = 0; k < 5; k++) if (v[k]) aadd(p + 2 + k, v[k]);
                return;
            }
        }
        if ((t & 7u) == 7u && ald(over)) return;
        s = (s + 1) & mask;
    }
    ast(over, 1u);                                                                       // the table is full
}

__global__ __launch_bounds__(kMetBlock) void k_metrics_fold(const void* __restrict__ recs, uint64_t n, MetDev M, const uint32_t* __restrict__ k8s_rows,
                                                            const uint2* __restrict__ net_rows) {
    __shared__ MetLds L;
    for (uint32_t k = threadIdx.x; k < kMetLdsSlots; k += kMetBlock) {
        L.a[k] = 0; L.b[k] = 0;
#pragma unroll
        for (int j = 0; j < 5; j++) L.sum[j][k] = 0;
    }
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * kMetBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kMetBlock + threadIdx.x; i < n; i += stride) {
        const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(recs) + i * kRecordBytes);
        const uint4 u2 = p[2], u3 = p[3], u4 = p[4];
        const uint64_t bytes = (uint64_t)u3.z | ((uint64_t)u3.w << 32), packets = u4.x;
        const uint32_t eth = u4.y & 0xffffu;
        const uint32_t is_ip = (eth == 0x0800u || eth == 0x86DDu) ? 1u : 0u;
        const uint32_t proto = is_ip ? (u2.y & 0xffu) : 0u;                              // a record that is not IP has no Proto key
        const uint2 kr = reinterpret_cast<const uint2*>(k8s_rows)[i];
        const uint2 nr = net_rows ? net_rows[i] : make_uint2(0xffffffffu, kNetNoDirection);
        uint32_t layer = 0;
        if (M.any_layer && M.has_layer) {                                                // FlpK8s::load_k8s
            bool app = false;
            if (kr.x < M.n_rows) app = (M.rows[kr.x].flags & kK8sRowApp) != 0;
            if (kr.y < M.n_rows) app = app || (M.rows[kr.y].flags & kK8sRowApp) != 0;
            layer = app ? 2u : 1u;
        }
        const uint64_t v[5] = {1ull, bytes, packets, bytes ? 1ull : 0ull, packets ? 1ull : 0ull};
        for (uint32_t g = 0; g < M.n_groupings; g++) {
            const uint32_t d = M.dims[g];
            const uint32_t* cs = M.cls[g][0];
            const uint32_t* cd = M.cls[g][1];
            const uint32_t sc = cs && kr.x < M.n_rows ? cs[kr.x] : 0u, dc = cd && kr.y < M.n_rows ? cd[kr.y] : 0u;
            const uint64_t ka = met_key_a(g, sc, dc);
            const uint64_t kb = met_key_b(g, (d & NFAGG_DIM_SRC_SUBNET_LABEL) ? nr.x & 0xffffu : kNetNoLabel,
                                          (d & NFAGG_DIM_DST_SUBNET_LABEL) ? nr.x >> 16 : kNetNoLabel,
                                          (d & NFAGG_DIM_FLOW_DIRECTION) ? nr.y & 0xffu : kNetNoDirection, (d & NFAGG_DIM_FLOW_LAYER) ? layer : 0u,
                                          (d & NFAGG_DIM_PROTO) ? proto : 0u, (d & NFAGG_DIM_PROTO) ? is_ip : 0u);
            uint32_t s = (uint32_t)met_hash(ka, kb) & (kMetLdsSlots - 1);
            bool done = false;
            for (uint32_t t = 0; t < kMetLdsProbe && !done; t++) {
                unsigned long long a = __hip_atomic_load(&L.a[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (a == 0) a = atomicCAS(&L.a[s], 0ull, (unsigned long long)ka);
                if (a == 0 || a == ka) {
                    unsigned long long b = __hip_atomic_load(&L.b[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (b == 0) b = atomicCAS(&L.b[s], 0ull, (unsigned long long)kb);
                    if (b == 0 || b == kb) {
#pragma unroll
                        for (int k = 0; k < 5; k++) if (v[k]) atomicAdd(&L.sum[k][s], (unsigned long long)v[k]);
                        done = true;
                    }
                }
                s = (s + 1) & (kMetLdsSlots - 1);
            }
            if (!done) met_global_add(M, g, ka, kb, v);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < kMetLdsSlots; k += kMetBlock) {
        const uint64_t ka = L.a[k];
        if (!ka) continue;
        const uint64_t v[5] = {L.sum[0][k], L.sum[1][k], L.sum[2][k], L.sum[3][k], L.sum[4][k]};
        met_global_add(M, met_key_grouping(ka), ka, L.b[k], v);
    }
}

// Which grouping block b of the concatenated tables belongs to.
NF_DEV uint32_t met_block_grouping(const MetDev& M, uint32_t b) {
    uint32_t g = 0;
    while (g + 1 < M.n_groupings && b >= M.first_block[g + 1]) g++;
    return g;
}

// One lane per slot of the concatenated tables: 1 for an occupied slot, scanned inside the block.
__global__ __launch_bounds__(kScanBlock) void k_metrics_count(MetDev M, uint32_t* __restrict__ local_off, uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t wave_tot[kScanBlock / 64];
    const uint32_t g = met_block_grouping(M, blockIdx.x);
    const uint32_t s = (blockIdx.x - M.first_block[g]) * kScanBlock + threadIdx.x;       // tables are multiples of kScanBlock slots
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint32_t occupied = M.slots[g][(size_t)s * kMetSlotWords] != 0 ? 1u : 0u;
    block_scan(occupied, i, (uint64_t)gridDim.x * kScanBlock, wave_tot, local_off, block_sum);
}

// block_base: the scan of the block sums over all groupings, the total last. Every lane works out the verdict from the
// groupings' counts; block 0 reports it; the groups are written only when no grouping is over.
__global__ __launch_bounds__(kScanBlock) void k_metrics_emit(MetDev M, const uint32_t* __restrict__ local_off, const uint64_t* __restrict__ block_base) {
    bool any_over = false;
    for (uint32_t g = 0; g < M.n_groupings; g++) {
        const uint32_t count = (uint32_t)(block_base[M.first_block[g + 1]] - block_base[M.first_block[g]]);
        const bool over = M.ctl->overflow[g] != 0 || count > M.cap[g];
        any_over = any_over || over;
        if (blockIdx.x == 0 && threadIdx.x == g) { M.ctl->count[g] = count; M.ctl->over[g] = over ? 1u : 0u; }
    }
    if (any_over) return;
    const uint32_t g = met_block_grouping(M, blockIdx.x);
    const uint32_t s = (blockIdx.x - M.first_block[g]) * kScanBlock + threadIdx.x;
    const uint4* q = reinterpret_cast<const uint4*>(M.slots[g] + (size_t)s * kMetSlotWords);
    const uint4 k = q[0];
    if ((k.x | k.y) == 0) return;
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const uint64_t at = block_base[blockIdx.x] - block_base[M.first_block[g]] + local_off[i];      // < count <= cap
    const uint64_t ka = (uint64_t)k.x | ((uint64_t)k.y << 32), kb = (uint64_t)k.z | ((uint64_t)k.w << 32);
    uint4* o = reinterpret_cast<uint4*>(M.out[g] + at);
    // nfagg_metric_group: src_class, dst_class, src_label | dst_label << 16, direction | layer << 8 | proto << 16 | is_ip << 24
    o[0] = make_uint4((uint32_t)ka & 0x1fffffffu, (uint32_t)(ka >> 29) & 0x1fffffffu, (uint32_t)kb,
                      ((uint32_t)(kb >> 32) & 0xffu) | (((uint32_t)(kb >> 40) & 3u) << 8) | (((uint32_t)(kb >> 42) & 0xffu) << 16) | (((uint32_t)(kb >> 50) & 1u) << 24));
    o[1] = q[1];
    o[2] = q[2];
    const uint4 last = q[3];
    o[3] = make_uint4(last.x, last.y, 0u, 0u);
}

hipError_t launch_metrics_fold(const void* d_recs, uint64_t n, const MetDev& M, const uint32_t* d_k8s_rows, const uint2* d_net_rows, hipStream_t s) {
    const uint64_t want = (n + kMetFlowsPerBlock - 1) / kMetFlowsPerBlock;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_metrics_fold, dim3((unsigned)(want < kMetMaxBlocks ? want : kMetMaxBlocks)), dim3(kMetBlock), 0, s, d_recs, n, M, d_k8s_rows, d_net_rows);
    return hipGetLastError();
}

hipError_t launch_metrics_emit(const MetDev& M, uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s) {
    const uint32_t blocks = M.first_block[M.n_groupings];
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_metrics_count, dim3(blocks), dim3(kScanBlock), 0, s, M, d_local_off, d_block_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_scan_block_sums(d_block_sum, blocks, d_block_base, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_metrics_emit, dim3(blocks), dim3(kScanBlock), 0, s, M, d_local_off, d_block_base);
    return hipGetLastError();
}

}  // namespace nfagg
