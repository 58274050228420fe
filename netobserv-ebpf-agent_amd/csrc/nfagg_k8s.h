// nfagg_k8s.h — the Kubernetes enrichment of the direct-FLP JSON line (flowlogs-pipeline transform network: add_kubernetes
// for SrcAddr and DstAddr, then add_kubernetes_infra; enrich.go:37-104,140-165), as a feature policy on top of FlpTls<Base>,
// and the kernel pair that runs it. The informers' answers come as the caller's table (nfagg_k8s_table_create): both
// sides' blocks of a row are rendered once on the host, a flow costs two probes of an open-addressed table (k_k8s_resolve,
// nfagg_k8s.hip) and a byte copy per block. Device code only; the table's layout is in nfagg_flp.h.
//   after DstAddr:     [,"DstK8S_HostIP":..,"DstK8S_Zone":..]   the dst row's block
//   after Interfaces:  [,"K8S_FlowLayer":"app"|"infra"]        with a layer
//   after SrcAddr:     [,"SrcK8S_HostIP":..,"SrcK8S_Zone":..]   the src row's block
#pragma once
#include "nfagg_tls.h"

namespace nfagg {

constexpr uint32_t kK8sLayerMax = sizeof(",\"K8S_FlowLayer\":\"infra\"") - 1;
constexpr uint32_t kK8sLineMax = 2 * kK8sMaxRendered + kK8sLayerMax;

// Row of the address w[0..3] (four little-endian dwords), kK8sNoRow when the table has none: linear probe from the
// hash's home slot; a step is the slot's two 16-byte halves, one aligned 32-byte read. The table is at most half full, so
// a probe ends at a free slot.
NF_DEV uint32_t k8s_probe(const K8sDev& K, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32), hi = (uint64_t)w2 | ((uint64_t)w3 << 32);
    uint32_t s = (uint32_t)k8s_hash(lo, hi) & K.mask;
    for (uint32_t t = 0; t <= K.mask; t++) {
        const uint4* p = reinterpret_cast<const uint4*>(K.slots + s);
        const uint4 key = p[0], val = p[1];
        if (val.x == kK8sNoRow) return kK8sNoRow;
        if (key.x == w0 && key.y == w1 && key.z == w2 && key.w == w3) return val.x;
        s = (s + 1) & K.mask;
    }
    return kK8sNoRow;
}

// FlpTls<Base> with the enrichment. The window takes what the longest line leaves of 32 KiB beside the wave's side LDS,
// as FlpTls sizes its own.
template <typename Base> struct FlpK8s : Base {
    static constexpr uint32_t kMaxLine = Base::kMaxLine + kK8sLineMax;
    static constexpr uint32_t kWindow = (32768 - Base::kSideLds - (kMaxLine + 15) / 16 * 16) / 16 * 16;
    static constexpr uint32_t kLds = kWindow + (kMaxLine + 15) / 16 * 16;
    static_assert(!Base::kDefers && kLds + Base::kSideLds <= 32768 && kWindow >= 16384, "four waves per compute unit, and a window worth its copy-out");
    const uint8_t* blob = nullptr;
    uint32_t off[2] = {}, len[2] = {};      // the src and the dst block: offset in 16-byte units, bytes (0: no row)
    uint32_t layer = 0;                     // 0: no key, 1: infra, 2: app

    // rows: the flow's two rows as k_k8s_resolve wrote them (kK8sNoRow for a record that is not IP: it has no address key)
    NF_DEV void load_k8s(const K8sDev& K, const uint32_t* __restrict__ rows, uint64_t i) {
        const uint2 r = reinterpret_cast<const uint2*>(rows)[i];
        const uint32_t row[2] = {r.x, r.y};
        blob = K.blob;
        bool app = false;
#pragma unroll
        for (int k = 0; k < 2; k++)
            if (row[k] < K.n_rows) {
                const uint4 m = reinterpret_cast<const uint4*>(K.rows)[row[k]];       // K8sRow
                off[k] = k ? m.y : m.x;
                len[k] = k ? m.z >> 16 : m.z & 0xffffu;
                app = app || (m.w & kK8sRowApp);
            }
        layer = K.has_layer ? (app ? 2u : 1u) : 0u;
    }
    template <typename S> NF_DEV void k8s_src(S& s) const { if (len[0]) put_blob(s, blob + (size_t)off[0] * 16, len[0]); }
    template <typename S> NF_DEV void k8s_dst(S& s) const { if (len[1]) put_blob(s, blob + (size_t)off[1] * 16, len[1]); }
    template <typename S> NF_DEV void k8s_layer(S& s) const {              // enrich.go:140-151
        if (layer == 2) lit(s, ",\"K8S_FlowLayer\":\"app\"");
        else if (layer == 1) lit(s, ",\"K8S_FlowLayer\":\"infra\"");
    }
};

// ---- the kernel pair: k_flp_size / k_flp_write (nfagg_flp_line.h) with the table and the flows' rows as two more
// arguments. Kernels of their own, so that the twelve instantiations of that pair stay what they are; Feat = FlpK8s<FlpTls<..>>,
// which never defers.
template <typename Feat>
__global__ __launch_bounds__(kScanBlock) void k_k8s_size(const void* __restrict__ recs, uint64_t n, FlpParams P, PbFeat F, TlsDev T, K8sDev K,
                                                         const uint32_t* __restrict__ k8s_rows, uint32_t* __restrict__ rows,
                                                         uint32_t* __restrict__ local_off, uint32_t* __restrict__ block_sum) {
    constexpr uint32_t kSlot = Feat::kSideLds >= 64 * 32 ? 32 : 0;
    __shared__ uint32_t wave_tot[kScanBlock / 64];
    __shared__ __align__(16) uint8_t name_lds[kSlot ? kScanBlock * kSlot : 16];
    __shared__ uint32_t tab_lds[kNamesLdsRows * (kNameRowBytes / 4)];
    const uint8_t* tab = stage_names<kScanBlock>(P.names, P.n_names, tab_lds);
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t len = 0;
    if (i < n) {
        Rec r;
        load_record(recs, i, r);
        uint32_t row[7];
        flp_rows(tab, P.n_names, r, row);
        Feat f;
        f.load(F, i, name_lds + threadIdx.x * kSlot);
        f.tls = T;
        f.load_k8s(K, k8s_rows, i);
        CountSink c;
        encode_line(c, r, P, row, f);
        len = c.n;
        uint4* o = reinterpret_cast<uint4*>(rows + i * 8);
        o[0] = make_uint4(row[0], row[1], row[2], row[3]);
        o[1] = make_uint4(row[4], row[5], row[6], len);
    }
    block_scan(len, i, n, wave_tot, local_off, block_sum);
}

template <typename Feat>
__global__ __launch_bounds__(64) void k_k8s_write(const void* __restrict__ recs, uint64_t n, FlpParams P, PbFeat F, TlsDev T, K8sDev K,
                                                  const uint32_t* __restrict__ k8s_rows, const uint32_t* __restrict__ rows,
                                                  const uint32_t* __restrict__ local_off, const uint64_t* __restrict__ block_base,
                                                  uint8_t* __restrict__ out, uint64_t* __restrict__ line_offsets) {
    constexpr uint32_t kSlot = Feat::kSideLds >= 64 * 32 ? 32 : 0;
    static_assert(Feat::kLds + Feat::kSideLds <= 32768, "four waves per compute unit");
    __shared__ __align__(16) uint8_t lds[Feat::kLds];
    __shared__ __align__(16) uint8_t name_lds[kSlot ? 64 * kSlot : 16];
    const uint64_t i0 = (uint64_t)blockIdx.x * 64, i = i0 + threadIdx.x;
    WaveImage w(block_base, local_off, i0);
    uint64_t my_off = 0; uint32_t my_len = 0;
    uint32_t row[7] = {};
    Rec r;
    Feat f;
    f.tls = T;
    if (i < n) {
        load_record(recs, i, r);
        const uint4* q = reinterpret_cast<const uint4*>(rows + i * 8);
        const uint4 a = q[0], b = q[1];
        row[0] = a.x; row[1] = a.y; row[2] = a.z; row[3] = a.w; row[4] = b.x; row[5] = b.y; row[6] = b.z;
        my_len = b.w;
        f.load(F, i, name_lds + threadIdx.x * kSlot);
        f.load_k8s(K, k8s_rows, i);
        my_off = record_off(block_base, local_off, i);
        line_offsets[i] = my_off;
        if (i == n - 1) line_offsets[n] = my_off + my_len;
    }
    w.close(my_off + my_len, out);
    const uint32_t p0 = w.pos(my_off);                            // my line = image bytes [p0, p0 + my_len)
    uint32_t lo = w.shift;
    while (lo < w.span) {                                         // the window loop of k_flp_write
        const uint32_t base = lo & ~15u;
        const bool mine = my_len && p0 >= lo && p0 - base < Feat::kWindow;
        if (mine) { FlpLds s{lds + (p0 - base)}; encode_line(s, r, P, row, f); }
        uint32_t hi = mine ? p0 + my_len : lo;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(hi, d, 64); hi = o > hi ? o : hi; }
        __syncthreads();
        copy_image_out(w.dst, lds, base, lo, hi);
        __syncthreads();
        lo = hi;
    }
}

template <typename Feat>
__attribute__((noinline)) hipError_t k8s_size_as(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat& F, const TlsDev& T, const K8sDev& K,
                                                 const uint32_t* d_k8s_rows, uint32_t* d_rows, uint32_t* d_local_off, uint32_t* d_block_sum,
                                                 uint64_t* d_block_base, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((n + kScanBlock - 1) / kScanBlock);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_k8s_size<Feat>, dim3(blocks), dim3(kScanBlock), 0, s, d_recs, n, P, F, T, K, d_k8s_rows, d_rows, d_local_off, d_block_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_block_sums(d_block_sum, blocks, d_block_base, s);
}
template <typename Feat>
__attribute__((noinline)) hipError_t k8s_write_as(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat& F, const TlsDev& T, const K8sDev& K,
                                                  const uint32_t* d_k8s_rows, const uint32_t* d_rows, const uint32_t* d_local_off,
                                                  const uint64_t* d_block_base, void* d_out, uint64_t* d_line_offsets, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_k8s_write<Feat>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d_recs, n, P, F, T, K, d_k8s_rows, d_rows, d_local_off,
                       d_block_base, (uint8_t*)d_out, d_line_offsets);
    return hipGetLastError();
}

}  // namespace nfagg
