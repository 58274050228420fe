// nfagg_ipfix.hip — evicted flow_record_t -> IPFIX messages (RFC 7011), in bulk on the GPU. Replaces, for the records
// Accounter.evict produces,
//   pkg/model/record.go:82-106       NewRecord (flow start/end wall-clock times, first-seen interface)
//   pkg/exporter/ipfix.go:264-383    setEntities / sendDataRecord / ExportFlows
//   go-ipfix exporter.SendSet        one message per flow: header, data set header, one data record (entities/ie.go encoders)
// Output: message i = out[msg_offsets[i], msg_offsets[i + 1]), one UDP datagram or one TCP write each.
//
// Layout (big-endian), v4 template: header@0 (version 10, length, export time, sequence, domain), set header@16
// (template id, length - 16), ethernetType@20 flowDirection@22 sourceMac@23 destinationMac@29 sourceIPv4@35
// destinationIPv4@39 protocol@43 ports@44/46 icmp type/code@48/49 octetDeltaCount@50 tcpControlBits@58
// flowStartSeconds@60 flowStartMilliseconds@64 flowEndSeconds@72 flowEndMilliseconds@76 packetDeltaCount@84
// interfaceName@92 (1-byte length + bytes): 93 + L bytes. The v6 template carries 16-byte addresses at 35/51 and
// shifts everything after them by 24: 117 + L bytes.
//
// Fixed layout, no varints: the size pass only has to resolve the interface name (kept as a row index for the write
// pass). The two-pass skeleton of nfagg_encode.h; its own: a wave's 64 messages (at most 64 x 133 B) fit one LDS
// image, written once through plain pointers.
#include "nfagg_encode.h"
#include "nfagg_ipfix.h"

namespace nfagg {

constexpr uint32_t kIpfixFixedV4 = 93, kIpfixFixedV6 = 117;          // message length without the name bytes
constexpr uint32_t kIpfixMaxMsg = kIpfixFixedV6 + 16;
constexpr uint32_t kIpfixImage = (64 * kIpfixMaxMsg + 15 + 15) / 16 * 16;   // 64 messages behind a shift of up to 15 bytes

NF_DEV uint32_t ipfix_len(uint32_t eth, uint32_t name_len) {          // model.IPv6Type picks the v6 template, anything else v4
    return (eth == 0x86DDu ? kIpfixFixedV6 : kIpfixFixedV4) + name_len;
}

// record.go:100-106: the first-seen interface is named for (if_index_first_seen, lMAC), lMAC = dst_mac when the first
// direction is 0 (ingress), src_mac otherwise. Returns row + 1 of the (sorted) table, 0 = unknown.
NF_DEV uint32_t ipfix_name_row(const uint8_t* tab, uint32_t n_names, const uint32_t (&d)[12], uint32_t& name_len, uint32_t unknown_len) {
    // d = record dwords 16..27
    const uint64_t smac = (uint64_t)d[2] | ((uint64_t)(d[3] & 0xffffu) << 32), dmac = (uint64_t)(d[3] >> 16) | ((uint64_t)d[4] << 16);
    const uint32_t dir = d[8] & 0xffu;
    const uint8_t* e = lookup_name(tab, n_names, d[5], mac_be(dir == 0 ? dmac : smac));
    name_len = e ? (uint32_t)e[11] : unknown_len;
    return e ? (uint32_t)((e - tab) / kNameRowBytes) + 1 : 0u;
}

// ---- kernel 1: message length per record (the name looked up once), block-local exclusive scan of the lengths
__global__ __launch_bounds__(kScanBlock) void k_ipfix_size(const void* __restrict__ recs, uint64_t n, IpfixParams P,
                                                           uint32_t* __restrict__ name_row, uint32_t* __restrict__ local_off,
                                                           uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t wave_tot[kScanBlock / 64];
    __shared__ uint32_t tab_lds[kNamesLdsRows * (kNameRowBytes / 4)];
    const uint8_t* tab = stage_names<kScanBlock>(P.names, P.n_names, tab_lds);
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t len = 0;
    if (i < n) {
        const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(recs) + i * kRecordBytes + 64);
        const uint4 a = p[0], b = p[1], c = p[2];            // record bytes 64..111: packets eth/flags macs if_index .. direction
        const uint32_t d[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        uint32_t nl;
        name_row[i] = ipfix_name_row(tab, P.n_names, d, nl, P.unknown_len);
        len = ipfix_len(d[1] & 0xffffu, nl);
    }
    block_scan(len, i, n, wave_tot, local_off, block_sum);
}

// big-endian N-byte value at p (LDS)
template <int N> NF_DEV void put_be(uint8_t* p, uint64_t v) {
#pragma unroll
    for (int k = 0; k < N; k++) p[k] = (uint8_t)(v >> (8 * (N - 1 - k)));
}
template <int OFF> NF_DEV uint8_t rec_byte(const Rec& r) { return (uint8_t)(r.d[OFF >> 2] >> (8 * (OFF & 3))); }

// One message at p: header, data set header, the data record of template v4 / v6 (ipfix.go:272-322 field by field).
NF_DEV void write_message(uint8_t* p, const Rec& r, const IpfixParams& P, uint32_t seq, uint32_t len, const uint32_t (&nw)[4], uint32_t nlen) {
    const uint32_t eth = r.eth();
    const bool v6 = eth == 0x86DDu;
    put_be<2>(p + 0, 10); put_be<2>(p + 2, len); put_be<4>(p + 4, P.export_time); put_be<4>(p + 8, seq); put_be<4>(p + 12, P.obs_domain);
    put_be<2>(p + 16, v6 ? P.tid_v6 : P.tid_v4); put_be<2>(p + 18, len - 16);
    put_be<2>(p + 20, eth);
    p[22] = (uint8_t)(r.d[24] & 0xffu);                                  // flowDirection = Interfaces[0].Direction
#pragma unroll
    for (int k = 0; k < 6; k++) p[23 + k] = (uint8_t)(r.d[(72 + k) >> 2] >> (8 * ((72 + k) & 3)));   // SrcMac, bytes as stored
#pragma unroll
    for (int k = 0; k < 6; k++) p[29 + k] = (uint8_t)(r.d[(78 + k) >> 2] >> (8 * ((78 + k) & 3)));   // DstMac
    const Ip4w sip{{r.d[0], r.d[1], r.d[2], r.d[3]}}, dip{{r.d[4], r.d[5], r.d[6], r.d[7]}};
    uint8_t* q;
    if (v6) {
#pragma unroll
        for (int k = 0; k < 16; k++) { p[35 + k] = ip_byte(sip, k); p[51 + k] = ip_byte(dip, k); }
        q = p + 67;
    } else {   // model.IP(..).To4(): the v4-mapped form (::ffff:a.b.c.d) gives a.b.c.d, anything else nil -> 0.0.0.0
        const bool sm = ip_v4_mapped(sip), dm = ip_v4_mapped(dip);
#pragma unroll
        for (int k = 0; k < 4; k++) { p[35 + k] = sm ? ip_byte(sip, 12 + k) : 0; p[39 + k] = dm ? ip_byte(dip, 12 + k) : 0; }
        q = p + 43;
    }
    // q: protocolIdentifier / nextHeaderIPv6 and everything after it (v4 offset - 43)
    q[0] = rec_byte<36>(r);
    q[1] = rec_byte<33>(r); q[2] = rec_byte<32>(r);                      // sourceTransportPort
    q[3] = rec_byte<35>(r); q[4] = rec_byte<34>(r);                      // destinationTransportPort
    q[5] = rec_byte<37>(r); q[6] = rec_byte<38>(r);                      // icmp type, code
    put_be<8>(q + 7, r.bytes());                                         // octetDeltaCount
    put_be<2>(q + 15, r.flags());                                        // tcpControlBits
    const TimeParts ts = flow_time(P.now_sec, P.now_nsec, P.mono_now, r.start());
    const TimeParts te = flow_time(P.now_sec, P.now_nsec, P.mono_now, r.end());
    put_be<4>(q + 17, (uint32_t)ts.sec);                                 // uint32(t.Unix())
    put_be<8>(q + 21, (uint64_t)(ts.sec * 1000 + ts.nsec / 1000000));    // uint64(t.UnixMilli())
    put_be<4>(q + 29, (uint32_t)te.sec);
    put_be<8>(q + 33, (uint64_t)(te.sec * 1000 + te.nsec / 1000000));
    put_be<8>(q + 41, r.packets());                                      // packetDeltaCount
    q[49] = (uint8_t)nlen;                                               // variable length: one length byte (< 255)
#pragma unroll
    for (int k = 0; k < 16; k++)
        if ((uint32_t)k < nlen) q[50 + k] = (uint8_t)(nw[k >> 2] >> (8 * (k & 3)));
}

// ---- kernel 3: write. One wave per 64 consecutive records; their messages are contiguous in the output.
__global__ __launch_bounds__(64) void k_ipfix_write(const void* __restrict__ recs, uint64_t n, IpfixParams P,
                                                    const uint32_t* __restrict__ name_row, const uint32_t* __restrict__ local_off,
                                                    const uint64_t* __restrict__ block_base, uint8_t* __restrict__ out,
                                                    uint64_t* __restrict__ msg_offsets) {
    __shared__ __align__(16) uint8_t img[kIpfixImage];
    const uint64_t i0 = (uint64_t)blockIdx.x * 64, i = i0 + threadIdx.x;
    WaveImage w(block_base, local_off, i0);
    uint64_t end = 0;
    if (i < n) {
        Rec r;
        load_record(recs, i, r);
        const uint32_t row = name_row[i];
        uint32_t nw[4] = {P.unknown_w[0], P.unknown_w[1], P.unknown_w[2], P.unknown_w[3]}, nlen = P.unknown_len;
        if (row) {   // the names at row + 12 are dword aligned (92-byte rows)
            const uint32_t* e = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(P.names) + (size_t)(row - 1) * kNameRowBytes);
            nlen = e[2] >> 24;
            nw[0] = e[3]; nw[1] = e[4]; nw[2] = e[5]; nw[3] = e[6];
        }
        const uint32_t len = ipfix_len(r.eth(), nlen);
        const uint64_t off = record_off(block_base, local_off, i);
        msg_offsets[i] = off;
        if (i == n - 1) msg_offsets[n] = off + len;
        end = off + len;
        write_message(img + w.pos(off), r, P, P.seq0 + (uint32_t)i, len, nw, nlen);
    }
    w.close(end, out);
    __syncthreads();
    copy_image_out(w.dst, img, 0, w.shift, w.span);
}

hipError_t launch_ipfix_size(const void* d_recs, uint64_t n, const IpfixParams& P, uint32_t* d_name_row, uint32_t* d_local_off,
                             uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((n + kScanBlock - 1) / kScanBlock);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ipfix_size, dim3(blocks), dim3(kScanBlock), 0, s, d_recs, n, P, d_name_row, d_local_off, d_block_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_block_sums(d_block_sum, blocks, d_block_base, s);
}

hipError_t launch_ipfix_write(const void* d_recs, uint64_t n, const IpfixParams& P, const uint32_t* d_name_row, const uint32_t* d_local_off,
                              const uint64_t* d_block_base, void* d_out, uint64_t* d_msg_offsets, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ipfix_write, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d_recs, n, P, d_name_row, d_local_off, d_block_base,
                       (uint8_t*)d_out, d_msg_offsets);
    return hipGetLastError();
}

}  // namespace nfagg
