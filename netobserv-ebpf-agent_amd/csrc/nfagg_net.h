// nfagg_net.h — three more rules of flowlogs-pipeline's transform network stage on the direct-FLP JSON line, as a feature
// policy on top of FlpK8s<FlpTls<Base>> and the kernel pair that runs it: reinterpret_direction
// (transform_network_direction.go:32-64), add_subnet_label for SrcAddr and DstAddr (transform_network.go:129-146,185-196)
// and decode_tcp_flags in place on Flags (transform_network.go:147-156, utils/tcp_flags.go:8-48). k_net_resolve
// (nfagg_net.hip) does the join ahead: encode_line sees two label indexes and a direction, and no table. Device code only;
// the table's layout is in nfagg_flp.h.
//   after DstPort:  [,"DstSubnetLabel":".."]      the dst label's fragment
//   Flags:          ["FIN","SYN",..] | null       in place of the number
//   after Flags:    [,"FlowDirection":0|1|2]
//   after SrcPort:  [,"SrcSubnetLabel":".."]      the src label's fragment
#pragma once
#include "nfagg_k8s.h"

namespace nfagg {

// What the rules add to a line at most: two fragments at the cap (18 bytes of key text, the quotes, the escaped label), the
// direction key, and the array of all eleven names where five digits were counted.
constexpr uint32_t kNetFlagNamesMax = sizeof("[\"FIN\",\"SYN\",\"RST\",\"PSH\",\"ACK\",\"URG\",\"ECE\",\"CWR\",\"SYN_ACK\",\"FIN_ACK\",\"RST_ACK\"]") - 1;
constexpr uint32_t kNetLineMax = 2 * kNetFragMax + (sizeof(",\"FlowDirection\":2") - 1) + kNetFlagNamesMax - 5;
static_assert(kNetFragMax == 20 + 256 && kNetFlagNamesMax == 79 && kNetLineMax == 552 + 18 + 74, "transform network keys");

// utils/tcp_flags.go:8-48: the names whose bit is set, in table order; no known bit: a nil slice, "null".
template <typename S> NF_DEV void tcp_flag_names(S& s, uint32_t v) {
    v &= 0x7ffu;
    if (!v) { lit(s, "null"); return; }
    if constexpr (is_count<S>::value) {                     // "NAME", per bit: 6 bytes for the eight three-letter names, 10 for the others
        s.n += 1 + 6 * (uint32_t)__popc(v & 0xffu) + 10 * (uint32_t)__popc(v >> 8);
    } else {
        uint8_t sep = '[';
#define NF_TCP_FLAG(bit, name) if (v & (bit)) { s.put(sep); sep = ','; lit(s, "\"" name "\""); }
        NF_TCP_FLAG(1u, "FIN") NF_TCP_FLAG(2u, "SYN") NF_TCP_FLAG(4u, "RST") NF_TCP_FLAG(8u, "PSH")
        NF_TCP_FLAG(16u, "ACK") NF_TCP_FLAG(32u, "URG") NF_TCP_FLAG(64u, "ECE") NF_TCP_FLAG(128u, "CWR")
        NF_TCP_FLAG(256u, "SYN_ACK") NF_TCP_FLAG(512u, "FIN_ACK") NF_TCP_FLAG(1024u, "RST_ACK")
#undef NF_TCP_FLAG
        s.put(']');
    }
}

// FlpK8s<..> with the three rules. The window takes what the longest line leaves of 32 KiB beside the wave's side LDS, as
// FlpK8s sizes its own.
template <typename Base> struct FlpNet : Base {
    static constexpr bool kFlagNames = true;
    static constexpr uint32_t kMaxLine = Base::kMaxLine + kNetLineMax;
    static constexpr uint32_t kWindow = (32768 - Base::kSideLds - (kMaxLine + 15) / 16 * 16) / 16 * 16;
    static constexpr uint32_t kLds = kWindow + (kMaxLine + 15) / 16 * 16;
    static_assert(!Base::kDefers && kLds + Base::kSideLds <= 32768 && kWindow >= 16384, "four waves per compute unit, and a window worth its copy-out");
    const uint8_t* net_blob = nullptr;
    uint32_t net_off[2] = {}, net_len[2] = {};   // the src and the dst fragment: offset in 16-byte units, bytes (0: no key)
    uint32_t dir = kNetNoDirection;
    bool names = false;                          // NFAGG_NET_DECODE_TCP_FLAGS

    // rows: the flow's nfagg_net_row as k_net_resolve wrote it
    NF_DEV void load_net(const NetDev& N, const uint2* __restrict__ rows, uint64_t i) {
        const uint2 r = rows[i];
        const uint32_t label[2] = {r.x & 0xffffu, r.x >> 16};
        net_blob = N.blob;
        dir = r.y & 0xffu;
        names = (N.flags & NFAGG_NET_DECODE_TCP_FLAGS) != 0;
#pragma unroll
        for (int k = 0; k < 2; k++)
            if (label[k] < N.n_labels) {
                const uint4 m = reinterpret_cast<const uint4*>(N.frags)[label[k]];        // NetFrag
                net_off[k] = k ? m.z : m.x;
                net_len[k] = k ? m.w : m.y;
            }
    }
    template <typename S> NF_DEV void src_subnet(S& s) const { if (net_len[0]) put_blob(s, net_blob + (size_t)net_off[0] * 16, net_len[0]); }
    template <typename S> NF_DEV void dst_subnet(S& s) const { if (net_len[1]) put_blob(s, net_blob + (size_t)net_off[1] * 16, net_len[1]); }
    template <typename S> NF_DEV void flow_direction(S& s) const {
        if (dir <= 2) { lit(s, ",\"FlowDirection\":"); s.put((uint8_t)('0' + dir)); }
    }
    template <typename S> NF_DEV void flags_value(S& s, uint32_t v) const {
        if (names) tcp_flag_names(s, v); else dec<5>(s, v);
    }
};

// ---- the kernel pair: k_k8s_size / k_k8s_write (nfagg_k8s.h) with the net table and the flows' net rows as two more
// arguments, under names of their own so that the eighteen instantiations of the two other pairs stay what they are.
// Feat = FlpNet<FlpK8s<FlpTls<..>>>, which never defers.
template <typename Feat>
__global__ __launch_bounds__(kScanBlock) void k_net_size(const void* __restrict__ recs, uint64_t n, FlpParams P, PbFeat F, TlsDev T, K8sDev K, NetDev N,
                                                         const uint32_t* __restrict__ k8s_rows, const uint2* __restrict__ net_rows,
                                                         uint32_t* __restrict__ rows, uint32_t* __restrict__ local_off,
                                                         uint32_t* __restrict__ block_sum) {
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
        f.load_net(N, net_rows, i);
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
__global__ __launch_bounds__(64) void k_net_write(const void* __restrict__ recs, uint64_t n, FlpParams P, PbFeat F, TlsDev T, K8sDev K, NetDev N,
                                                  const uint32_t* __restrict__ k8s_rows, const uint2* __restrict__ net_rows,
                                                  const uint32_t* __restrict__ rows, const uint32_t* __restrict__ local_off,
                                                  const uint64_t* __restrict__ block_base, uint8_t* __restrict__ out,
                                                  uint64_t* __restrict__ line_offsets) {
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
        f.load_net(N, net_rows, i);
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
__attribute__((noinline)) hipError_t net_size_as(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat& F, const TlsDev& T, const K8sDev& K,
                                                 const NetDev& N, const uint32_t* d_k8s_rows, const uint2* d_net_rows, uint32_t* d_rows,
                                                 uint32_t* d_local_off, uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((n + kScanBlock - 1) / kScanBlock);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_net_size<Feat>, dim3(blocks), dim3(kScanBlock), 0, s, d_recs, n, P, F, T, K, N, d_k8s_rows, d_net_rows, d_rows, d_local_off,
                       d_block_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_block_sums(d_block_sum, blocks, d_block_base, s);
}
template <typename Feat>
__attribute__((noinline)) hipError_t net_write_as(const void* d_recs, uint64_t n, const FlpParams& P, const PbFeat& F, const TlsDev& T, const K8sDev& K,
                                                  const NetDev& N, const uint32_t* d_k8s_rows, const uint2* d_net_rows, const uint32_t* d_rows,
                                                  const uint32_t* d_local_off, const uint64_t* d_block_base, void* d_out, uint64_t* d_line_offsets,
                                                  hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_net_write<Feat>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d_recs, n, P, F, T, K, N, d_k8s_rows, d_net_rows, d_rows,
                       d_local_off, d_block_base, (uint8_t*)d_out, d_line_offsets);
    return hipGetLastError();
}

}  // namespace nfagg
