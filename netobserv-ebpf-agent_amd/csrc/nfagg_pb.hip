// nfagg_pb.hip — evicted flow_record_t -> serialized pbflow.Record, in bulk on the GPU
// (SURVEY.md §8(f) rank 1). Replaces, for the records Accounter.evict produces,
//   pkg/model/record.go:82-125      NewRecord (flow start/end wall-clock times, interface list)
//   pkg/pbflow/proto.go:18-149      FlowsToPB / FlowToPB
//   proto.Marshal of pbflow.Record  (pkg/exporter/kafka_proto.go:53, grpc marshalling of pbflow.Records)
//   pkg/exporter/kafka_proto.go:37-47 getFlowKey
// Output: for record i the frame `0x0A varint(len) body` at frame_offsets[i]; any run of frames
// [a, b) is a serialized pbflow.Records{entries[a..b)} (proto/flow.proto:16-18, what GRPCProto sends,
// split at will for GRPC_MESSAGE_MAX_FLOWS); the body alone is the Kafka message value.
// Wire rules as google.golang.org/protobuf applies them: fields in field-number order, proto3
// scalars omitted at zero, message fields emitted whenever FlowToPB sets the pointer (DataLink,
// Network, Transport, both Timestamps, agent_ip, time_flow_rtt = durationpb.New(0) -> empty message),
// oneof members emitted even at their zero value (IP.ipv4 = 0).
//
// With a PbFeat the same kernels encode the MapTracer branch (pkg/flow/tracer_map.go:103-146): the
// full model.BpfFlowContent — DNS, packet drops, xlat, RTT/IPsec, QUIC (proto.go:79-118,129-138;
// record.go:116-125) — with a nil SampleDecoder (record.go:126): network events are not decoded.
// The NE instantiations (PbFeat::ne_rows given, the *_netev entry points) add field 27, network_events_metadata
// (proto.go:140-147): the rendered NetworkEvent of each table row nfagg_netev_resolve found for the flow. The
// kernels without the hook are separate instantiations and keep their code and their registers.
//
// Byte-granular, HBM-bound streaming work: 144 B read + ~110 B written per record (more with
// features). The two-pass skeleton of nfagg_encode.h; its own: a wave's image is encoded one fixed
// window at a time (8, 16 or 24 KiB), the whole encoder running once per window the wave's frames span.
#include "nfagg_encode.h"
#include "nfagg_pb.h"

namespace nfagg {

NF_DEV uint32_t varint_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 0x80) { v >>= 7; n++; }
    return n;
}
template <typename S> NF_DEV void put_varint(S& s, uint64_t v) {
    while (v >= 0x80) { s.put((uint8_t)(v | 0x80)); v >>= 7; }
    s.put((uint8_t)v);
}
template <typename S> NF_DEV void put_tag(S& s, uint32_t field, uint32_t wt) { put_varint(s, ((uint64_t)field << 3) | wt); }
template <typename S> NF_DEV void put_uint(S& s, uint32_t field, uint64_t v) { if (v) { put_tag(s, field, 0); put_varint(s, v); } }
NF_DEV uint32_t uint_len(uint32_t field, uint64_t v) { return v ? varint_len((uint64_t)field << 3) + varint_len(v) : 0; }

// message IP { oneof { fixed32 ipv4 = 1; bytes ipv6 = 2; } } as a sub-message of `field`
// The address travels as an Ip4w (nfagg_encode.h).
template <typename S> NF_DEV void put_ip(S& s, uint32_t field, const Ip4w& ip, bool v6) {
    put_tag(s, field, 2);
    if (v6) {
        s.put(18); s.put(0x12); s.put(16);
#pragma unroll
        for (int k = 0; k < 16; k++) s.put(ip_byte(ip, k));
    } else {   // model.IntEncodeV4 (record.go:202-204): big-endian value of the last four bytes; fixed32 is little-endian on the wire
        s.put(5); s.put(0x0D);
        s.put(ip_byte(ip, 15)); s.put(ip_byte(ip, 14)); s.put(ip_byte(ip, 13)); s.put(ip_byte(ip, 12));
    }
}

// google.protobuf.Timestamp of flow_time (record.go:90-97, proto.go:61-68)
template <typename S> NF_DEV void put_time(S& s, uint32_t field, const TimeParts& t) {
    put_tag(s, field, 2);
    s.put((uint8_t)(uint_len(1, (uint64_t)t.sec) + uint_len(2, (uint64_t)t.nsec)));
    put_uint(s, 1, (uint64_t)t.sec);      // int64: a negative value takes ten bytes
    put_uint(s, 2, (uint64_t)t.nsec);
}

// message DupMapEntry { string interface = 1; Direction direction = 2; string udn = 3; } as Record.dup_list (26)
template <typename S> NF_DEV void put_dup(S& s, const PbParams& P, const uint8_t* tab, uint32_t if_index, uint64_t mac48, uint32_t dir) {
    const uint8_t* e = lookup_name(tab, P.n_names, if_index, mac48);
    const uint32_t lens = e ? *reinterpret_cast<const uint32_t*>(e + 8) : 0u;      // bytes 8..11: mac[4..5], has_mac, name_len
    const uint32_t nlen = e ? lens >> 24 : P.unknown_len;
    const uint32_t ulen = e ? e[28] : 0u;
    const uint32_t body = (nlen ? 2 + nlen : 0) + uint_len(2, dir) + (ulen ? 2 + ulen : 0);
    put_tag(s, 26, 2);
    s.put((uint8_t)body);                  // < 128 by the table's field widths
    if (nlen) {
        s.put(0x0A); s.put((uint8_t)nlen);
        if (e) { for (uint32_t k = 0; k < nlen; k++) s.put(e[12 + k]); }
        else { for (uint32_t k = 0; k < nlen; k++) s.put((uint8_t)P.unknown[k]); }
    }
    put_uint(s, 2, dir);
    if (ulen) { s.put(0x1A); s.put((uint8_t)ulen); for (uint32_t k = 0; k < ulen; k++) s.put(e[29 + k]); }
}

// google.protobuf.Duration = durationpb.New(time.Duration(d)): secs = d / 1e9 truncating, nanos = d - secs*1e9,
// both carry the sign; Nanos is an int32 (a negative one is sign-extended to a ten-byte varint).
template <typename S> NF_DEV void put_duration(S& s, uint32_t field, uint64_t d_u) {
    const int64_t d = (int64_t)d_u, secs = d / 1000000000ll;
    const uint64_t nanos = (uint64_t)(int64_t)(int32_t)(d - secs * 1000000000ll);
    put_tag(s, field, 2);
    s.put((uint8_t)(uint_len(1, (uint64_t)secs) + uint_len(2, nanos)));
    put_uint(s, 1, (uint64_t)secs);
    put_uint(s, 2, nanos);
}

// The body of pbflow.Record for one flow: evicted record `r`, plus the feature parts of flow `i` when F carries
// them — each part is read whole with vector loads before anything is emitted. `name_lds`: 32 bytes of LDS owned by
// this lane (the DNS name is walked byte by byte). Same code sizes (CountSink) and writes (WindowSink).
template <bool NE, typename S> NF_DEV void encode_record(S& s, const Rec& r, const PbParams& P, const PbFeat& F, uint64_t i, uint8_t* name_lds, const uint8_t* tab) {
    const uint32_t have = F.present ? F.present[i] : 0u;
    const bool add = F.additional && (have & 1u), dns = F.dns && (have & 2u), drp = F.drops && (have & 4u);
    const bool xlt = F.xlat && (have & 16u), quc = F.quic && (have & 32u);
    uint32_t addw[8] = {}, dnsw[16] = {}, drpw[8] = {}, xltw[14] = {}, qucw[6] = {};
    if (add) load_dwords16(F.additional + i * 32, addw);     // start@0 end@8 flow_rtt@16 ipsec_ret@24 eth@28 ipsec_encrypted@30
    if (dns) load_dwords16(F.dns + i * 64, dnsw);            // latency@16 id@24 flags@26 eth@28 errno@30 name@31..62
    if (drp) load_dwords16(F.drops + i * 32, drpw);          // bytes@16 packets@18 cause@20 flags@24 eth@26 state@28
    if (xlt) load_dwords8(F.xlat + i * 56, xltw);            // saddr@16 daddr@32 sport@48 dport@50 zone@52
    if (quc) load_dwords8(F.quic + i * 24, qucw);            // version@16 eth@20 long@22 short@23
    if (dns) {
#pragma unroll
        for (int k = 0; k < 32; k++) name_lds[k] = (uint8_t)(dnsw[(31 + k) >> 2] >> (8 * ((31 + k) & 3)));
    }
    const uint32_t eth = r.eth();
    const uint32_t dirn = r.d[24] & 0xffu;
    put_uint(s, 1, eth);
    put_uint(s, 2, dirn);
    put_time(s, 3, flow_time(P.now_sec, P.now_nsec, P.mono_now, r.start()));
    put_time(s, 4, flow_time(P.now_sec, P.now_nsec, P.mono_now, r.end()));
    const uint64_t smac = mac_be(r.smac()), dmac = mac_be(r.dmac());
    put_tag(s, 5, 2); s.put((uint8_t)(uint_len(1, smac) + uint_len(2, dmac)));
    put_uint(s, 1, smac); put_uint(s, 2, dmac);
    {   // Network: addresses by eth_protocol (proto.go:125-139), dscp
        const bool v6 = eth == 0x86DDu;    // model.IPv6Type
        const Ip4w sip{{r.d[0], r.d[1], r.d[2], r.d[3]}}, dip{{r.d[4], r.d[5], r.d[6], r.d[7]}};
        const uint32_t ipl = v6 ? 20 : 7;   // tag + len + body of one IP sub-message
        put_tag(s, 6, 2); s.put((uint8_t)(2 * ipl + uint_len(3, r.dscp())));
        put_ip(s, 1, sip, v6); put_ip(s, 2, dip, v6);
        put_uint(s, 3, r.dscp());
    }
    {   // Transport
        const uint32_t sp = r.d[8] & 0xffffu, dp = r.d[8] >> 16, pr = r.d[9] & 0xffu;
        put_tag(s, 7, 2); s.put((uint8_t)(uint_len(1, sp) + uint_len(2, dp) + uint_len(3, pr)));
        put_uint(s, 1, sp); put_uint(s, 2, dp); put_uint(s, 3, pr);
    }
    put_uint(s, 8, r.bytes());
    put_uint(s, 9, r.packets());
    put_ip(s, 12, Ip4w{{P.agent_ip_w[0], P.agent_ip_w[1], P.agent_ip_w[2], P.agent_ip_w[3]}}, !P.agent_is_v4);
    put_uint(s, 13, r.flags());
    put_uint(s, 14, (r.d[9] >> 8) & 0xffu);      // icmp_type
    put_uint(s, 15, (r.d[9] >> 16) & 0xffu);     // icmp_code
    if (drp) {                                   // proto.go:92-98
        const uint32_t bp = drpw[4], fe = drpw[6];
        put_uint(s, 16, bp & 0xffffu); put_uint(s, 17, bp >> 16);
        put_uint(s, 18, fe & 0xffffu); put_uint(s, 19, drpw[7] & 0xffu);
        put_uint(s, 20, drpw[5]);
    }
    if (dns) {                                   // proto.go:79-91, record.go:116-120
        const uint32_t idf = dnsw[6];
        put_uint(s, 21, idf & 0xffffu); put_uint(s, 22, idf >> 16);
        const uint64_t lat = (uint64_t)dnsw[4] | ((uint64_t)dnsw[5] << 32);
        if (lat) put_duration(s, 23, lat);
    }
    put_duration(s, 24, add ? ((uint64_t)addw[4] | ((uint64_t)addw[5] << 32)) : 0ull);   // time_flow_rtt = durationpb.New(fr.TimeFlowRtt): always present
    if (dns) put_uint(s, 25, (dnsw[7] >> 16) & 0xffu);
    {   // dup_list = record.Interfaces (record.go:100-114)
        const uint64_t lmac = mac_be(dirn == 0 ? r.dmac() : r.smac());
        put_dup(s, P, tab, r.d[21], lmac, dirn);
        uint32_t nb = r.d[24] >> 24; if (nb > 6) nb = 6;
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t od = k < 4 ? (r.d[25] >> (8 * k)) & 0xffu : (r.d[26] >> (8 * (k - 4))) & 0xffu;
            uint32_t oi = r.d[27];
#pragma unroll
            for (int q = 1; q < 6; q++) oi = ((uint32_t)q == k) ? r.d[27 + q] : oi;
            put_dup(s, P, tab, oi, lmac, od);
        }
    }
    if constexpr (NE) {                          // network_events_metadata = 27 (proto.go:140-147), tag bytes 0xDA 0x01
        uint32_t ev[4];
        netev_rows(F.ne_rows, i, ev);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (ev[k] < F.ne_n) {
                const uint4 m = netev_row_blobs(F.ne_tab, ev[k]);
                put_tag(s, 27, 2); put_varint(s, m.z >> 16);
                put_blob(s, F.ne_blob + m.y, m.z >> 16);
            }
    }
    if (xlt) {                                   // proto.go:99-105,129-138: address family by the FLOW's eth_protocol
        const bool v6 = eth == 0x86DDu;
        const uint32_t sd = xltw[12], ze = xltw[13];
        const uint32_t ipl = v6 ? 20 : 7;
        put_tag(s, 28, 2);
        s.put((uint8_t)(2 * ipl + uint_len(3, sd & 0xffffu) + uint_len(4, sd >> 16) + uint_len(5, ze & 0xffffu)));
        put_ip(s, 1, Ip4w{{xltw[4], xltw[5], xltw[6], xltw[7]}}, v6); put_ip(s, 2, Ip4w{{xltw[8], xltw[9], xltw[10], xltw[11]}}, v6);
        put_uint(s, 3, sd & 0xffffu); put_uint(s, 4, sd >> 16); put_uint(s, 5, ze & 0xffffu);
    }
    put_uint(s, 29, r.sampling());
    if (add) {                                   // proto.go:106-111
        put_uint(s, 30, ((addw[7] >> 16) & 0xffu) ? 1u : 0u);
        put_uint(s, 31, (uint64_t)(int64_t)(int32_t)addw[6]);
    }
    if (dns) {                                   // dns_name = 32
        CountSink c;
        const uint32_t nl = dns_dotted<false>(c, name_lds);
        if (nl) { put_tag(s, 32, 2); s.put((uint8_t)nl); dns_dotted<true>(s, name_lds); }
    }
    put_uint(s, 33, r.d[33] & 0xffffu);          // ssl_version
    put_uint(s, 34, (r.d[34] >> 24) & 1u);       // HasSSLMismatch (record.go:255-257)
    put_uint(s, 35, (r.d[34] >> 16) & 0xffu);    // tls_types
    put_uint(s, 36, r.d[33] >> 16);              // tls_cipher_suite
    put_uint(s, 37, r.d[34] & 0xffffu);          // tls_key_share
    if (quc) {                                   // proto.go:112-118
        const uint32_t ver = qucw[4], lh = (qucw[5] >> 16) & 0xffu, sh = qucw[5] >> 24;
        put_tag(s, 38, 2);
        s.put((uint8_t)(uint_len(1, ver) + uint_len(2, lh) + uint_len(3, sh)));
        put_uint(s, 1, ver); put_uint(s, 2, lh); put_uint(s, 3, sh);
    }
}

// ---- kernel 1: body length per record, frame length, block-local exclusive scan of the frame lengths
template <bool NE>
__global__ __launch_bounds__(kScanBlock) void k_pb_size(const void* __restrict__ recs, uint64_t n, PbParams P, PbFeat F,
                                                        uint32_t* __restrict__ body_len, uint32_t* __restrict__ local_off,
                                                        uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t wave_tot[kScanBlock / 64];
    __shared__ __align__(4) uint8_t name_lds[kScanBlock][32];
    __shared__ uint32_t tab_lds[kNamesLdsRows * (kNameRowBytes / 4)];
    const uint8_t* tab = stage_names<kScanBlock>(P.names, P.n_names, tab_lds);
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t frame = 0;
    if (i < n) {
        Rec r;
        load_record(recs, i, r);
        r.canonicalize();
        CountSink c;
        encode_record<NE>(c, r, P, F, i, name_lds[threadIdx.x], tab);
        body_len[i] = c.n;
        frame = 1 + varint_len(c.n) + c.n;
    }
    block_scan(frame, i, n, wave_tot, local_off, block_sum);
}

// ---- kernel 3: encode. One wave per 64 consecutive records, one kPbWindow-byte window of its output at a time.
// The window (LDS per wave, beside 2 KiB of DNS-name slots and the 8.6 KiB namer table) is chosen by the host from the
// average frame length the size pass found: the whole encoder runs once per window a wave's 64 frames span, so the
// window should hold them all (64 x ~110 B for Accounter records, 64 x ~270 B with every feature part).
// (a frame is at most 1033 bytes, DESIGN.md §4.7a, 3097 with four network events at their cap; the window sink takes a
// frame of any length: a frame that straddles windows is encoded once per window)

template <uint32_t kPbWindow, bool NE = false>
__global__ __launch_bounds__(64) void k_pb_write(const void* __restrict__ recs, uint64_t n, PbParams P, PbFeat F,
                                                 const uint32_t* __restrict__ body_len, const uint32_t* __restrict__ local_off,
                                                 const uint64_t* __restrict__ block_base, uint8_t* __restrict__ out,
                                                 uint64_t* __restrict__ frame_offsets, uint8_t* __restrict__ kafka_keys) {
    __shared__ __align__(16) unsigned char lds[kPbWindow];
    __shared__ __align__(4) uint8_t name_lds[64][32];
    __shared__ uint32_t tab_lds[kNamesLdsRows * (kNameRowBytes / 4)];
    const uint8_t* tab = stage_names<64>(P.names, P.n_names, tab_lds);
    const uint64_t i0 = (uint64_t)blockIdx.x * 64, i = i0 + threadIdx.x;
    WaveImage w(block_base, local_off, i0);
    uint64_t my_off = 0; uint32_t my_len = 0, bl = 0;
    Rec r;
    if (i < n) {
        load_record(recs, i, r);
        r.canonicalize();
        my_off = record_off(block_base, local_off, i);
        bl = body_len[i];
        my_len = 1 + varint_len(bl) + bl;
        frame_offsets[i] = my_off;
        if (kafka_keys) {
            // getFlowKey (kafka_proto.go:37-47): the two 16-byte addresses, the smaller one first
            int c = 0;
            for (int k = 0; k < 16 && c == 0; k++) {
                const int a = (r.d[k / 4] >> (8 * (k & 3))) & 0xff, b = (r.d[4 + k / 4] >> (8 * (k & 3))) & 0xff;
                c = a - b;
            }
            uint4* kk = reinterpret_cast<uint4*>(kafka_keys + i * 32);
            const uint4 sip = make_uint4(r.d[0], r.d[1], r.d[2], r.d[3]), dip = make_uint4(r.d[4], r.d[5], r.d[6], r.d[7]);
            kk[0] = c <= 0 ? sip : dip; kk[1] = c <= 0 ? dip : sip;
        }
        if (i == n - 1) frame_offsets[n] = my_off + my_len;
    }
    w.close(my_off + my_len, out);
    const uint32_t p0 = w.pos(my_off);                            // my frame = image bytes [p0, p0 + my_len)
    for (uint32_t lo = 0; lo < w.span; lo += kPbWindow) {
        const uint32_t hi = lo + kPbWindow < w.span ? lo + kPbWindow : w.span;
        if (my_len && p0 < hi && p0 + my_len > lo) {
            WindowSink s{lds, p0, lo, hi - lo};
            s.put(0x0A);                                          // Records.entries = 1, length-delimited
            put_varint(s, bl);
            encode_record<NE>(s, r, P, F, i, name_lds[threadIdx.x], tab);
        }
        __syncthreads();
        copy_image_out(w.dst, lds, lo, w.shift, hi);              // from max(lo, shift): lo is 0 or beyond any shift
        __syncthreads();
    }
}

hipError_t launch_pb_size(const void* d_recs, uint64_t n, const PbParams& P, const PbFeat& F, uint32_t* d_body_len, uint32_t* d_local_off,
                          uint32_t* d_block_sum, uint64_t* d_block_base, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((n + kScanBlock - 1) / kScanBlock);
    (void)hipGetLastError();
    if (F.ne_rows) hipLaunchKernelGGL(k_pb_size<true>, dim3(blocks), dim3(kScanBlock), 0, s, d_recs, n, P, F, d_body_len, d_local_off, d_block_sum);
    else hipLaunchKernelGGL(k_pb_size<false>, dim3(blocks), dim3(kScanBlock), 0, s, d_recs, n, P, F, d_body_len, d_local_off, d_block_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_block_sums(d_block_sum, blocks, d_block_base, s);
}

// One window rule for both sets of instantiations; F.ne_rows picks the set that carries the network-events hook.
hipError_t launch_pb_write(const void* d_recs, uint64_t n, const PbParams& P, const PbFeat& F, const uint32_t* d_body_len, const uint32_t* d_local_off,
                           const uint64_t* d_block_base, void* d_out, uint64_t* d_frame_offsets, void* d_kafka_keys, uint64_t total_bytes, hipStream_t s) {
    const uint64_t avg = n ? total_bytes / n : 0;
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    const bool ne = F.ne_rows != nullptr;
    void (*kernel)(const void*, uint64_t, PbParams, PbFeat, const uint32_t*, const uint32_t*, const uint64_t*, uint8_t*, uint64_t*, uint8_t*);
    if (avg <= 120) kernel = ne ? k_pb_write<8192, true> : k_pb_write<8192>;
    else if (avg <= 248) kernel = ne ? k_pb_write<16384, true> : k_pb_write<16384>;
    else kernel = ne ? k_pb_write<24576, true> : k_pb_write<24576>;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel, grid, block, 0, s, d_recs, n, P, F, d_body_len, d_local_off, d_block_base, (uint8_t*)d_out, d_frame_offsets, (uint8_t*)d_kafka_keys);
    return hipGetLastError();
}

}  // namespace nfagg
