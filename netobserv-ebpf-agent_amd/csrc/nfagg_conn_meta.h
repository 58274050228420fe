// nfagg_conn_meta.h — the flow logs of flowlogs-pipeline's extract conntrack stage on the direct-FLP JSON line, as a feature
// policy on top of FlpNet<FlpK8s<FlpTls<Base>>> and the kernel pair that runs it. The stage drops every flow its filter
// turns away (conntrack.go:70-74) and adds two keys to the others (conntrack.go:120-126, 281-287):
//   an untracked flow:   no line (a zero-length one: line_offsets[i + 1] == line_offsets[i])
//   a tracked flow:      ,"_HashId":"<hex>","_RecordType":"flowLog"      in front of the closing brace
// Tracked is encode_line's `ports` condition and the one k_conn_claim (nfagg_conn.hip) applies: an IP ethertype and protocol
// 6, 17 or 132. It is read from the record, never from the id: a tracked flow's total may be 0. <hex> is
// strconv.FormatUint(id, 16). The ids are what nfagg_conn_fold wrote for these records. Device code only.
#pragma once
#include "nfagg_net.h"

namespace nfagg {

constexpr uint32_t kConnMetaLineMax = (sizeof(",\"_HashId\":\"\",\"_RecordType\":\"flowLog\"") - 1) + 16;
static_assert(kConnMetaLineMax == 53, "extract conntrack's two keys");

NF_DEV bool conn_tracked(const Rec& r) {
    const uint32_t eth = r.eth(), proto = r.d[9] & 0xffu;
    return (eth == 0x0800u || eth == 0x86DDu) && (proto == 6 || proto == 17 || proto == 132);
}

// strconv.FormatUint(v, 16): lower case, no padding, "0" for 0
template <typename S> NF_DEV void hex_u64(S& s, uint64_t v) {
    const uint32_t nd = v ? (uint32_t)(67 - __clzll((long long)v)) / 4u : 1u;
    if constexpr (is_count<S>::value) s.n += nd;
    else {
#pragma unroll
        for (int k = 15; k >= 0; k--)
            if ((uint32_t)k < nd) s.put(hexc((uint32_t)(v >> (4 * k)) & 15u));
    }
}

// FlpNet<..> with the two keys. The window takes what the longest line leaves of 32 KiB beside the wave's side LDS, as FlpNet
// sizes its own. All three bases leave at least 16 384.
template <typename Base> struct FlpConnMeta : Base {
    static constexpr uint32_t kMaxLine = Base::kMaxLine + kConnMetaLineMax;
    static constexpr uint32_t kWindow = (32768 - Base::kSideLds - (kMaxLine + 15) / 16 * 16) / 16 * 16;
    static constexpr uint32_t kLds = kWindow + (kMaxLine + 15) / 16 * 16;
    static_assert(!Base::kDefers && kLds + Base::kSideLds <= 32768 && kWindow >= 16384, "four waves per compute unit, and a window worth its copy-out");
    uint64_t hash_id = 0;

    template <typename S> NF_DEV void conn_meta(S& s) const {
        lit(s, ",\"_HashId\":\""); hex_u64(s, hash_id); lit(s, "\",\"_RecordType\":\"flowLog\"");
    }
};

// ---- the kernel pair: k_net_size / k_net_write (nfagg_net.h) with the flows' hash ids as one more argument, under names of
// their own so that the instantiations of the three other pairs stay what they are. An untracked flow is measured as 0 and
// never encoded; the window loop of the write kernel already passes over a lane without a line.
template <typename Feat>
__global__ __launch_bounds__(kScanBlock) void k_connlog_size(const void* __restrict__ recs, uint64_t n, FlpParams P, PbFeat F, TlsDev T, K8sDev K, NetDev N,
                                                             const uint32_t* __restrict__ k8s_rows, const uint2* __restrict__ net_rows,
                                                             const uint64_t* __restrict__ hash_ids, uint32_t* __restrict__ rows,
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
        uint32_t row[7] = {};
        if (conn_tracked(r)) {
            flp_rows(tab, P.n_names, r, row);
            Feat f;
            f.load(F, i, name_lds + threadIdx.x * kSlot);
            f.tls = T;
            f.load_k8s(K, k8s_rows, i);
            f.load_net(N, net_rows, i);
            f.hash_id = hash_ids[i];
            CountSink c;
            encode_line(c, r, P, row, f);
            len = c.n;
        }
        uint4* o = reinterpret_cast<uint4*>(rows + i * 8);
        o[0] = make_uint4(row[0], row[1], row[2], row[3]);
        o[1] = make_uint4(row[4], row[5], row[6], len);
    }
    block_scan(len, i, n, wave_tot, local_off, block_sum);
}

template <typename Feat>
__global__ __launch_bounds__(64) void k_connlog_write(const void* __restrict__ recs, uint64_t n, FlpParams P, PbFeat F, TlsDev T, K8sDev K, NetDev N,
                                                      const uint32_t* __restrict__ k8s_rows, const uint2* __restrict__ net_rows,
                                                      const uint64_t* __restrict__ hash_ids, const uint32_t* __restrict__ rows,
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
        my_len = b.w;                                                 // 0: an untracked flow, whose parts and rows are not read
        if (my_len) {
            f.load(F, i, name_lds + threadIdx.x * kSlot);
            f.load_k8s(K, k8s_rows, i);
            f.load_net(N, net_rows, i);
            f.hash_id = hash_ids[i];
        }
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
__attribute__((noinline)) hipError_t connlog_size_as(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat& F, const TlsDev& T, const K8sDev& K,
                                                     const NetDev& N, const uint32_t* d_k8s_rows, const uint2* d_net_rows, const uint64_t* d_hash_ids,
                                                     uint32_t* d_rows, uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base,
                                                     hipStream_t s) {
    const uint32_t blocks = (uint32_t)((n + kScanBlock - 1) / kScanBlock);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_connlog_size<Feat>, dim3(blocks), dim3(kScanBlock), 0, s, d_recs, n, P, F, T, K, N, d_k8s_rows, d_net_rows, d_hash_ids, d_rows,
                       d_local_off, d_block_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_block_sums(d_block_sum, blocks, d_block_base, s);
}
template <typename Feat>
__attribute__((noinline)) hipError_t connlog_write_as(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat& F, const TlsDev& T, const K8sDev& K,
                                                      const NetDev& N, const uint32_t* d_k8s_rows, const uint2* d_net_rows, const uint64_t* d_hash_ids,
                                                      const uint32_t* d_rows, const uint32_t* d_local_off, const uint64_t* d_block_base, void* d_out,
                                                      uint64_t* d_line_offsets, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_connlog_write<Feat>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d_recs, n, P, F, T, K, N, d_k8s_rows, d_net_rows,
                       d_hash_ids, d_rows, d_local_off, d_block_base, (uint8_t*)d_out, d_line_offsets);
    return hipGetLastError();
}

}  // namespace nfagg
