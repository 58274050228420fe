// nfagg_flp_ipfix.hip — flowlogs-pipeline's `write ipfix` (pkg/pipeline/write/write_ipfix.go) on the device: the enriched flow
// as one IPFIX message per flow, with the writer's carried element state (include/nfagg.h, "write ipfix on the device").
//
// createDataRecord mutates one element list per family; a key that is absent from a flow's map leaves the value of the last
// flow of the family that had it. So flow i's bytes depend on earlier flows. Five kernels:
//   k_ipfix_carry       one lane per flow: the family and a bit per carry group (presence); inside the wave the source of every
//                       group is a ballot masked to the flow's family and to the lanes at or before it, and a count of leading
//                       zeros; across the block's waves a running last over per-wave aggregates in LDS; per block one aggregate
//                       per (family, group)
//   k_ipfix_carry_scan  the running last over the blocks' aggregates (k_scan_block_sums' pattern: chunks, their sums, fix-up)
//   k_ipfix_size        closes the sources that lie before the flow's block, gathers the values from their source flows (or the
//                       state), measures the message with the code that writes it, decides sent / failed, and scans the lengths
//                       and the sent flags inside the block (nfagg_encode.h)
//   k_ipfix_write       one wave per 64 flows: the messages in an LDS image, copied out 16 bytes at a time; a wave whose
//                       messages exceed the image (long strings) writes to global memory directly
//   k_ipfix_state       what the last flow of each family, and the last setter of each group, leave behind: the state the next
//                       call starts from, string bytes owned
// The sources are STORED (16 x 4 bytes per flow): both later passes need them, and recomputing them means the
// ballots and the block prefix twice more plus the presence inputs (feature parts, rows) read three times.
#include "nfagg_flp_line.h"
#include "nfagg_flp_ipfix.h"

namespace nfagg {

constexpr uint32_t kIxImage = 32768;           // 64 messages of 512 bytes; DESIGN.md §4.7q
constexpr uint32_t kIxXlatBytes = sizeof(nfagg_xlat_metrics), kIxAddBytes = sizeof(nfagg_additional_metrics);
static_assert(kIxXlatBytes == 56 && kIxAddBytes == 32, "feature part layouts");
static_assert(sizeof(nfagg_flp_ipfix_elements) == 9424 && offsetof(nfagg_flp_ipfix_elements, str) == 208, "state layout");

NF_DEV Ip4w ix_load_ip(const uint8_t* p) { const uint32_t* q = reinterpret_cast<const uint32_t*>(p); return Ip4w{{q[0], q[1], q[2], q[3]}}; }
// string k of the six: which side's row (0 src, 1 dst) and which of its three strings (0 namespace, 1 name, 2 host name)
NF_DEV uint32_t ix_str_side(uint32_t k) { return k < 4 ? k >> 1 : k - 4; }
NF_DEV uint32_t ix_str_field(uint32_t k) { return k < 4 ? k & 1u : 2u; }

// The xlat keys of flow j (decode_protobuf.go:155-168): the part is present and neither address is AllZeroIP.
NF_DEV bool ix_xlat(const IxArgs& A, uint64_t j, Ip4w& xs, Ip4w& xd, uint32_t& ports) {
    if (!A.F.xlat || !A.F.present || !(A.F.present[j] & NFAGG_FEAT_XLAT)) return false;
    const uint8_t* x = A.F.xlat + j * kIxXlatBytes;
    xs = ix_load_ip(x + 16); xd = ix_load_ip(x + 32);
    ports = *reinterpret_cast<const uint32_t*>(x + 48);           // sport | dport << 16
    return !ip_all_zero(xs) && !ip_all_zero(xd);
}
NF_DEV uint64_t ix_rtt(const IxArgs& A, uint64_t j) {             // record.go:121-125: 0 = no TimeFlowRttNs key
    if (!A.F.additional || !A.F.present || !(A.F.present[j] & NFAGG_FEAT_ADDITIONAL)) return 0;
    return *reinterpret_cast<const uint64_t*>(A.F.additional + j * kIxAddBytes + 16);
}

// The group bits of flow i: which conditionally absent keys its map has.
NF_DEV uint32_t ix_presence(const IxArgs& A, const Rec& r, uint64_t i) {
    const uint32_t eth = r.eth(), proto = r.d[9] & 0xffu;
    const bool ip = eth == 0x0800u || eth == 0x86DDu;
    uint32_t b = 0;
    if (r.bytes()) b |= 1u << kIxBytes;
    if (r.packets()) b |= 1u << kIxPackets;
    if (r.sampling()) b |= 1u << kIxSampling;
    if (ip) {
        b |= 1u << kIxAddr;
        if (proto == 1 || proto == 58) b |= 1u << kIxIcmp;
        else if (proto == 6 || proto == 17 || proto == 132) { b |= 1u << kIxPorts; if (proto == 6) b |= 1u << kIxFlags; }
    }
    Ip4w xs, xd; uint32_t xp = 0;
    if (ix_xlat(A, i, xs, xd, xp)) { if (xp & 0xffffu) b |= 1u << kIxXlatSrcPort; if (xp >> 16) b |= 1u << kIxXlatDstPort; }
    if (A.enterprise) {                                            // elements of the enterprise part of the templates only
        if (ix_rtt(A, i)) b |= 1u << kIxRtt;
        if (A.k8s_rows) {
            const uint2 rw = reinterpret_cast<const uint2*>(A.k8s_rows)[i];
            const uint32_t row[2] = {rw.x, rw.y};
#pragma unroll
            for (uint32_t k = 0; k < 6; k++) {
                const uint32_t rr = row[ix_str_side(k)];
                if (rr < A.n_srows && ((A.srows[rr].present >> ix_str_field(k)) & 1u)) b |= 1u << (kIxStr0 + k);
            }
        }
    }
    return b;
}

// ---- kernel 1: presence and the carry inside a block
__global__ __launch_bounds__(kScanBlock) void k_ipfix_carry(IxArgs A, uint32_t stride) {
    __shared__ int32_t wagg[kScanBlock / 64][2 * kIxAggs];
    __shared__ int32_t wpre[kScanBlock / 64][2 * kIxAggs];
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool valid = i < A.n;
    uint32_t bits = 0; bool v6 = false;
    if (valid) {
        Rec r;
        load_record(A.recs, i, r);
        bits = ix_presence(A, r, i) | (1u << kIxAny);
        v6 = r.eth() == 0x86DDu;
        A.meta[i] = (bits & 0xffffu) | (v6 ? kIxMetaV6 : 0u);
    }
    const uint64_t mf = __ballot(valid && v6);
    const uint64_t le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);          // the lanes at or before mine
    const int32_t wave_i0 = (int32_t)(i - (uint64_t)lane);
    int32_t mine[kIxGroups];
#pragma unroll
    for (uint32_t g = 0; g < kIxAggs; g++) {
        const uint64_t m = __ballot(valid && ((bits >> g) & 1u));
        const uint64_t m0 = m & ~mf, m1 = m & mf;
        if (lane == 0) {
            wagg[wave][g] = m0 ? wave_i0 + 63 - (int32_t)__builtin_clzll(m0) : -1;
            wagg[wave][kIxAggs + g] = m1 ? wave_i0 + 63 - (int32_t)__builtin_clzll(m1) : -1;
        }
        if (g < kIxGroups) {
            const uint64_t mm = (v6 ? m1 : m0) & le;
            mine[g] = mm ? wave_i0 + 63 - (int32_t)__builtin_clzll(mm) : kIxOpen;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * kIxAggs) {                                          // the running last over the block's 16 waves
        int32_t run = -1;
        for (int w = 0; w < kScanBlock / 64; w++) { wpre[w][threadIdx.x] = run; const int32_t x = wagg[w][threadIdx.x]; if (x >= 0) run = x; }
        A.agg[(size_t)threadIdx.x * stride + blockIdx.x] = run;
    }
    __syncthreads();
    if (valid) {
        const uint32_t f = v6 ? kIxAggs : 0u;
#pragma unroll
        for (uint32_t g = 0; g < kIxGroups; g++)
            if (mine[g] == kIxOpen) { const int32_t p = wpre[wave][f + g]; if (p >= 0) mine[g] = p; }
        int4* o = reinterpret_cast<int4*>(A.src + i * kIxGroups);
#pragma unroll
        for (int q = 0; q < 4; q++) o[q] = make_int4(mine[4 * q], mine[4 * q + 1], mine[4 * q + 2], mine[4 * q + 3]);
    }
}

// ---- kernel 2: pre[fg][b] = the last flow with (family, group) set before block b; pre[fg][blocks] = in the whole call
__global__ __launch_bounds__(kIxScanThreads) void k_ipfix_carry_scan(const int32_t* __restrict__ agg, int32_t* __restrict__ pre,
                                                                    uint32_t blocks, uint32_t stride) {
    __shared__ int32_t part[kIxScanThreads];
    const int32_t* a = agg + (size_t)blockIdx.x * stride;
    int32_t* p = pre + (size_t)blockIdx.x * stride;
    const uint32_t per = (blocks + kIxScanThreads - 1) / kIxScanThreads;
    const uint32_t lo = threadIdx.x * per, hi = lo + per < blocks ? lo + per : blocks;
    int32_t run = -1;
    for (uint32_t k = lo; k < hi; k++) if (a[k] >= 0) run = a[k];
    part[threadIdx.x] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t acc = -1;
        for (uint32_t k = 0; k < kIxScanThreads; k++) { const int32_t x = part[k]; part[k] = acc; if (x >= 0) acc = x; }
        p[blocks] = acc;
    }
    __syncthreads();
    int32_t acc = part[threadIdx.x];
    for (uint32_t k = lo; k < hi; k++) { p[k] = acc; if (a[k] >= 0) acc = a[k]; }
}

// ---- the values of one message: every carried element from its source flow or the state
struct IxMsg {
    Ip4w sip, dip, xs, xd;
    uint32_t proto, itype, icode, sport, dport, flags, xsp, xdp, selalg;
    uint64_t bytes, packets, rtt, prob;
    const uint8_t* kp[6]; uint32_t kl[6];
    bool v6, xset, fail;
};

NF_DEV void ix_gather(const IxArgs& A, const Rec& r, uint64_t i, const int32_t (&src)[kIxGroups], bool v6, IxMsg& M) {
    const nfagg_flp_ipfix_elements* st = A.state + (v6 ? 1 : 0);
    const uint32_t* R = reinterpret_cast<const uint32_t*>(A.recs);
    const int32_t me = (int32_t)i;
#define IX_RD(j, dw) ((j) == me ? r.d[dw] : R[(size_t)(j) * kRecordDwords + (dw)])
    M.v6 = v6;
    int32_t j = src[kIxBytes];
    M.bytes = j < 0 ? st->bytes : ((uint64_t)IX_RD(j, 14) | ((uint64_t)IX_RD(j, 15) << 32));
    j = src[kIxPackets];
    M.packets = j < 0 ? st->packets : (uint64_t)IX_RD(j, 16);
    j = src[kIxSampling];
    if (j < 0) { M.selalg = st->selector_algorithm; M.prob = (uint64_t)__double_as_longlong(st->sampling_probability); }
    else { M.selalg = 4; M.prob = (uint64_t)__double_as_longlong(1.0 / (double)IX_RD(j, 23)); }     // IEEE division: no fast-math in this build
    j = src[kIxAddr];
    bool addr_ok = true;
    if (j < 0) { addr_ok = st->addr_set != 0; M.sip = ix_load_ip(st->src_addr); M.dip = ix_load_ip(st->dst_addr); M.proto = st->proto; }
    else {
        M.sip = Ip4w{{IX_RD(j, 0), IX_RD(j, 1), IX_RD(j, 2), IX_RD(j, 3)}};
        M.dip = Ip4w{{IX_RD(j, 4), IX_RD(j, 5), IX_RD(j, 6), IX_RD(j, 7)}};
        M.proto = IX_RD(j, 9) & 0xffu;
    }
    j = src[kIxIcmp];
    if (j < 0) { M.itype = st->icmp_type; M.icode = st->icmp_code; } else { const uint32_t w = IX_RD(j, 9); M.itype = (w >> 8) & 0xffu; M.icode = (w >> 16) & 0xffu; }
    j = src[kIxPorts];
    if (j < 0) { M.sport = st->src_port; M.dport = st->dst_port; } else { const uint32_t w = IX_RD(j, 8); M.sport = w & 0xffffu; M.dport = w >> 16; }
    j = src[kIxFlags];
    M.flags = j < 0 ? st->flags : ((IX_RD(j, 17) >> 16) & A.flags_mask);
#undef IX_RD
    uint32_t xp = 0;
    M.xset = ix_xlat(A, i, M.xs, M.xd, xp);                        // the addresses are the flow's own or the Default
    j = src[kIxXlatSrcPort];
    M.xsp = j < 0 ? st->xlat_src_port : (uint32_t)*reinterpret_cast<const uint16_t*>(A.F.xlat + (size_t)j * kIxXlatBytes + 48);
    j = src[kIxXlatDstPort];
    M.xdp = j < 0 ? st->xlat_dst_port : (uint32_t)*reinterpret_cast<const uint16_t*>(A.F.xlat + (size_t)j * kIxXlatBytes + 50);
    j = src[kIxRtt];
    M.rtt = j < 0 ? st->rtt_ns : *reinterpret_cast<const uint64_t*>(A.F.additional + (size_t)j * kIxAddBytes + 16);
#pragma unroll
    for (uint32_t k = 0; k < 6; k++) {
        j = src[kIxStr0 + k];
        if (j < 0) { M.kp[k] = reinterpret_cast<const uint8_t*>(st->str[1 + k]); M.kl[k] = st->str_len[1 + k]; }
        else {
            const IxStrRow& row = A.srows[A.k8s_rows[2 * (size_t)j + ix_str_side(k)]];     // in range: the group bit was set from it
            M.kp[k] = A.sblob + row.off[ix_str_field(k)]; M.kl[k] = row.len[ix_str_field(k)];
        }
    }
    // entities/ie.go:683-688: an Ipv4Address element whose value has no To4() fails the record
    M.fail = !v6 && (!addr_ok || !ip_v4_mapped(M.sip) || !ip_v4_mapped(M.dip) || (M.xset && (!ip_v4_mapped(M.xs) || !ip_v4_mapped(M.xd))));
}

template <int N, typename S> NF_DEV void ix_be(S& s, uint64_t v) {
    if constexpr (is_count<S>::value) s.n += N;
    else {
#pragma unroll
        for (int k = 0; k < N; k++) s.put((uint8_t)(v >> (8 * (N - 1 - k))));
    }
}
template <typename S> NF_DEV void ix_ip16(S& s, const Ip4w& a) {
    if constexpr (is_count<S>::value) s.n += 16;
    else {
#pragma unroll
        for (int k = 0; k < 16; k++) s.put(ip_byte(a, k));
    }
}
template <typename S> NF_DEV void ix_ip4(S& s, const Ip4w& a) {    // To4() of a v4-mapped address
    if constexpr (is_count<S>::value) s.n += 4;
    else {
#pragma unroll
        for (int k = 12; k < 16; k++) s.put(ip_byte(a, k));
    }
}
template <typename S> NF_DEV void ix_mac(S& s, uint64_t mac) {     // byte 0 in the low bits
    if constexpr (is_count<S>::value) s.n += 6;
    else {
#pragma unroll
        for (int k = 0; k < 6; k++) s.put((uint8_t)(mac >> (8 * k)));
    }
}
// entities/ie.go:695-708: one length byte below 255 bytes, else 0xFF and two
template <typename S> NF_DEV void ix_str_prefix(S& s, uint32_t len) {
    if (len < 255) s.put((uint8_t)len); else { s.put(0xff); s.put((uint8_t)(len >> 8)); s.put((uint8_t)len); }
}
// len bytes at p, 16-byte aligned with the bytes up to the next multiple of 16 readable (the blob's and the state's slots)
template <typename S> NF_DEV void ix_str(S& s, const uint8_t* p, uint32_t len) {
    ix_str_prefix(s, len);
    esc_str(s, p, len);
}
// the name of namer row `row` (row of the sorted table + 1; 0: the unknown name): its length and four words
NF_DEV uint32_t ix_name(const IxArgs& A, uint32_t row, uint32_t (&w)[4]) {
    if (!row) { w[0] = A.unknown_w[0]; w[1] = A.unknown_w[1]; w[2] = A.unknown_w[2]; w[3] = A.unknown_w[3]; return A.unknown_len; }
    const uint32_t* e = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(A.names) + (size_t)(row - 1) * kNameRowBytes);
    w[0] = e[3]; w[1] = e[4]; w[2] = e[5]; w[3] = e[6];
    return e[2] >> 24;
}
template <typename S> NF_DEV void ix_name_bytes(S& s, const uint32_t (&w)[4], uint32_t len) {
    if constexpr (is_count<S>::value) s.n += len;
    else {
#pragma unroll
        for (int k = 0; k < 16; k++) if ((uint32_t)k < len) s.put((uint8_t)(w[k >> 2] >> (8 * (k & 3))));
    }
}

// One message: header (exporter/msg.go), set header (entities/set.go), the data record in template order. The same code
// measures (CountSink; `len` and `seq` are not known yet and not looked at) and writes.
template <typename S>
NF_DEV void ix_encode(S& s, const IxArgs& A, const Rec& r, const IxMsg& M, const uint32_t (&row)[7], uint32_t seq, uint32_t len) {
    ix_be<2>(s, 10); ix_be<2>(s, len); ix_be<4>(s, A.export_time); ix_be<4>(s, seq); ix_be<4>(s, A.obs_domain);
    ix_be<2>(s, M.v6 ? A.tid_v6 : A.tid_v4); ix_be<2>(s, len - 16);
    const Ip4w zero{{0, 0, 0, 0}};
    if (M.v6) {
        ix_ip16(s, M.sip); ix_ip16(s, M.dip);
        ix_be<1>(s, M.proto);                                      // nextHeaderIPv6: Proto
        ix_be<1>(s, M.itype); ix_be<1>(s, M.icode);
        ix_ip16(s, M.xset ? M.xs : zero); ix_ip16(s, M.xset ? M.xd : zero);      // Default: net.IPv6zero
    } else {
        ix_ip4(s, M.sip); ix_ip4(s, M.dip);
        ix_be<1>(s, M.itype); ix_be<1>(s, M.icode);
        ix_ip4(s, M.xset ? M.xs : zero); ix_ip4(s, M.xset ? M.xd : zero);        // Default: net.IPv4zero
    }
    ix_be<2>(s, r.eth());
    ix_be<1>(s, flp_dir(r, 0));                                     // flowDirection: uint8(IfDirections[0])
    ix_mac(s, r.smac()); ix_mac(s, r.dmac());
    ix_be<1>(s, M.proto);
    ix_be<2>(s, M.sport); ix_be<2>(s, M.dport);
    ix_be<8>(s, M.bytes);
    const TimeParts ts = flow_time(A.now_sec, A.now_nsec, A.mono_now, r.start());
    const TimeParts te = flow_time(A.now_sec, A.now_nsec, A.mono_now, r.end());
    ix_be<8>(s, (uint64_t)(ts.sec * 1000 + ts.nsec / 1000000));    // uint64(TimeFlowStartMs)
    ix_be<8>(s, (uint64_t)(te.sec * 1000 + te.nsec / 1000000));
    ix_be<8>(s, M.packets);
    const uint32_t ni = flp_n_intf(r);
    uint32_t nw[7][4], nl[7];
    uint32_t joined = ni - 1, dirs = ni - 1;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        nl[k] = 0;
        if ((uint32_t)k < ni) { nl[k] = ix_name(A, row[k], nw[k]); joined += nl[k]; dirs += ndigits<3>(flp_dir(r, k)); }
    }
    s.put((uint8_t)nl[0]); ix_name_bytes(s, nw[0], nl[0]);         // interfaceName: Interfaces[0], at most 16 bytes
    ix_be<2>(s, M.flags);
    ix_be<2>(s, M.xsp); ix_be<2>(s, M.xdp);
    ix_be<2>(s, M.selalg); ix_be<8>(s, M.prob);
    if (A.enterprise) {
#pragma unroll
        for (int k = 0; k < 6; k++) ix_str(s, M.kp[k], M.kl[k]);
        ix_be<8>(s, M.rtt);
        s.put((uint8_t)joined);                                    // interfaces: strings.Join(ifs, ","), at most 7 * 16 + 6 bytes
#pragma unroll
        for (int k = 0; k < 7; k++)
            if ((uint32_t)k < ni) { if (k) s.put(','); ix_name_bytes(s, nw[k], nl[k]); }
        s.put((uint8_t)dirs);                                      // directions: strconv.Itoa of each, joined
#pragma unroll
        for (int k = 0; k < 7; k++)
            if ((uint32_t)k < ni) { if (k) s.put(','); dec<3>(s, flp_dir(r, k)); }
    }
}

NF_DEV void ix_load_src(const IxArgs& A, uint64_t i, int32_t (&src)[kIxGroups]) {
    const int4* p = reinterpret_cast<const int4*>(A.src + i * kIxGroups);
#pragma unroll
    for (int q = 0; q < 4; q++) { const int4 v = p[q]; src[4 * q] = v.x; src[4 * q + 1] = v.y; src[4 * q + 2] = v.z; src[4 * q + 3] = v.w; }
}

// ---- kernel 3: sources closed, the message measured, sent or failed, the two block scans
__global__ __launch_bounds__(kScanBlock) void k_ipfix_flp_size(IxArgs A, uint32_t stride) {
    __shared__ uint32_t wave_tot[kScanBlock / 64], wave_sent[kScanBlock / 64];
    __shared__ uint32_t tab_lds[kNamesLdsRows * (kNameRowBytes / 4)];
    const uint8_t* tab = stage_names<kScanBlock>(A.names, A.n_names, tab_lds);
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t len = 0, sent = 0;
    if (i < A.n) {
        Rec r;
        load_record(A.recs, i, r);
        const uint32_t meta = A.meta[i];
        const bool v6 = (meta & kIxMetaV6) != 0;
        int32_t src[kIxGroups];
        ix_load_src(A, i, src);
        bool changed = false;
#pragma unroll
        for (uint32_t g = 0; g < kIxGroups; g++)
            if (src[g] == kIxOpen) { src[g] = A.pre[(size_t)((v6 ? kIxAggs : 0u) + g) * stride + blockIdx.x]; changed = true; }
        if (changed) {
            int4* o = reinterpret_cast<int4*>(A.src + i * kIxGroups);
#pragma unroll
            for (int q = 0; q < 4; q++) o[q] = make_int4(src[4 * q], src[4 * q + 1], src[4 * q + 2], src[4 * q + 3]);
        }
        uint32_t row[7];
        flp_rows(tab, A.n_names, r, row);
        IxMsg M;
        ix_gather(A, r, i, src, v6, M);
        CountSink c;
        ix_encode(c, A, r, M, row, 0, 0);
        const uint32_t st = M.fail ? NFAGG_FLP_IPFIX_FAIL_FAMILY : c.n > A.max_msg ? NFAGG_FLP_IPFIX_FAIL_SIZE : NFAGG_FLP_IPFIX_SENT;
        A.meta[i] = meta | (st << kIxMetaStatusShift);               // the caller's status array is written by the write pass alone
        sent = st == NFAGG_FLP_IPFIX_SENT ? 1u : 0u;
        len = sent ? c.n : 0u;
        uint4* o = reinterpret_cast<uint4*>(A.rows + i * 8);
        o[0] = make_uint4(row[0], row[1], row[2], row[3]);
        o[1] = make_uint4(row[4], row[5], row[6], len);
    }
    block_scan(len, i, A.n, wave_tot, A.local_off, A.block_sum);
    block_scan(sent, i, A.n, wave_sent, A.seq_local, A.seq_sum);
}

// ---- kernel 4: write. One wave per 64 consecutive flows; their messages are contiguous in the output.
__global__ __launch_bounds__(64) void k_ipfix_flp_write(IxArgs A, uint8_t* __restrict__ out, uint64_t* __restrict__ msg_offsets,
                                                        uint8_t* __restrict__ status) {
    __shared__ __align__(16) uint8_t img[kIxImage + 16];
    const uint64_t i0 = (uint64_t)blockIdx.x * 64, i = i0 + threadIdx.x;
    WaveImage w(A.block_base, A.local_off, i0);
    uint64_t my_off = 0; uint32_t len = 0;
    uint32_t row[7] = {}, meta = 0;
    if (i < A.n) {
        meta = A.meta[i];
        status[i] = (uint8_t)((meta >> kIxMetaStatusShift) & 3u);
        const uint4* q = reinterpret_cast<const uint4*>(A.rows + i * 8);
        const uint4 a = q[0], b = q[1];
        row[0] = a.x; row[1] = a.y; row[2] = a.z; row[3] = a.w; row[4] = b.x; row[5] = b.y; row[6] = b.z;
        len = b.w;
        my_off = record_off(A.block_base, A.local_off, i);
        msg_offsets[i] = my_off;
        if (i == A.n - 1) msg_offsets[A.n] = my_off + len;
    }
    w.close(i < A.n ? my_off + len : 0, out);
    const bool fits = w.span <= kIxImage;                          // wave-uniform
    if (len) {
        Rec r;
        load_record(A.recs, i, r);
        int32_t src[kIxGroups];
        ix_load_src(A, i, src);
        IxMsg M;
        ix_gather(A, r, i, src, (meta & kIxMetaV6) != 0, M);
        const uint32_t seq = A.seq0 + (uint32_t)(A.seq_base[i / kScanBlock] + A.seq_local[i]);
        FlpLds s{(fits ? img : w.dst) + w.pos(my_off)};             // w.dst + w.pos(off) == out + off
        ix_encode(s, A, r, M, row, seq, len);
    }
    if (fits) {
        __syncthreads();
        copy_image_out(w.dst, img, 0, w.shift, w.span);
    }
}

// ---- kernel 5: the state the call leaves. One block per family; thread 0 sets the values, the block copies the strings.
__global__ __launch_bounds__(256) void k_ipfix_state(IxArgs A, uint32_t blocks, uint32_t stride) {
    __shared__ const uint8_t* sp[NFAGG_FLP_IPFIX_N_STRINGS];
    __shared__ uint32_t sl[NFAGG_FLP_IPFIX_N_STRINGS];
    __shared__ uint8_t text[3][128];                               // interfaceName, interfaces, directions
    const uint32_t f = blockIdx.x;
    nfagg_flp_ipfix_elements* st = A.state + f;
    const int32_t* last = A.pre + (size_t)f * kIxAggs * stride + blocks;       // last[g * stride]
    const int32_t any = last[(size_t)kIxAny * stride];
    if (any < 0) return;                                           // no flow of this family: nothing moved (block-uniform)
    if (threadIdx.x == 0) {
        Rec r;
        load_record(A.recs, (uint64_t)any, r);
        // the elements every flow sets: Etype, IfDirections, the MACs, the times, Interfaces, the postNAT addresses (or their Default)
        st->etype = (uint16_t)r.eth(); st->flow_direction = (uint8_t)flp_dir(r, 0); st->mac_set = 1;
        for (int k = 0; k < 6; k++) { st->src_mac[k] = (uint8_t)(r.smac() >> (8 * k)); st->dst_mac[k] = (uint8_t)(r.dmac() >> (8 * k)); }
        const TimeParts ts = flow_time(A.now_sec, A.now_nsec, A.mono_now, r.start());
        const TimeParts te = flow_time(A.now_sec, A.now_nsec, A.mono_now, r.end());
        st->start_ms = (uint64_t)(ts.sec * 1000 + ts.nsec / 1000000); st->end_ms = (uint64_t)(te.sec * 1000 + te.nsec / 1000000);
        Ip4w xs, xd; uint32_t xp = 0;
        const bool xset = ix_xlat(A, (uint64_t)any, xs, xd, xp);
        st->xlat_set = 1;
        for (int k = 0; k < 16; k++) {                             // Default: IPv4zero (To16: ::ffff:0.0.0.0) / IPv6zero
            const uint8_t z = (f == 0 && (k == 10 || k == 11)) ? 0xff : 0;
            st->xlat_src_addr[k] = xset ? ip_byte(xs, k) : z; st->xlat_dst_addr[k] = xset ? ip_byte(xd, k) : z;
        }
        uint32_t row[7];
        flp_rows(reinterpret_cast<const uint8_t*>(A.names), A.n_names, r, row);
        const uint32_t ni = flp_n_intf(r);
        uint32_t n1 = 0, n2 = 0;
        for (uint32_t k = 0; k < ni; k++) {
            uint32_t w[4];
            const uint32_t nl = ix_name(A, row[k], w);
            if (k) { text[1][n1++] = ','; text[2][n2++] = ','; }
            for (uint32_t c = 0; c < nl; c++) { const uint8_t b = (uint8_t)(w[c >> 2] >> (8 * (c & 3))); text[1][n1++] = b; if (k == 0) text[0][c] = b; }
            if (k == 0) sl[0] = nl;
            FlpLds d{text[2] + n2};
            dec<3>(d, flp_dir(r, (int)k));
            n2 = (uint32_t)(d.p - text[2]);
        }
        sp[0] = text[0]; sp[7] = text[1]; sl[7] = n1; sp[8] = text[2]; sl[8] = n2;
        const uint32_t* R = reinterpret_cast<const uint32_t*>(A.recs);
        int32_t j;
        if ((j = last[(size_t)kIxBytes * stride]) >= 0) st->bytes = (uint64_t)R[(size_t)j * kRecordDwords + 14] | ((uint64_t)R[(size_t)j * kRecordDwords + 15] << 32);
        if ((j = last[(size_t)kIxPackets * stride]) >= 0) st->packets = R[(size_t)j * kRecordDwords + 16];
        if ((j = last[(size_t)kIxSampling * stride]) >= 0) { st->selector_algorithm = 4; st->sampling_probability = 1.0 / (double)R[(size_t)j * kRecordDwords + 23]; }
        if ((j = last[(size_t)kIxAddr * stride]) >= 0) {
            const uint8_t* b = reinterpret_cast<const uint8_t*>(R + (size_t)j * kRecordDwords);
            for (int k = 0; k < 16; k++) { st->src_addr[k] = b[k]; st->dst_addr[k] = b[16 + k]; }
            st->proto = b[36]; st->addr_set = 1;
        }
        if ((j = last[(size_t)kIxIcmp * stride]) >= 0) { const uint32_t w = R[(size_t)j * kRecordDwords + 9]; st->icmp_type = (uint8_t)(w >> 8); st->icmp_code = (uint8_t)(w >> 16); }
        if ((j = last[(size_t)kIxPorts * stride]) >= 0) { const uint32_t w = R[(size_t)j * kRecordDwords + 8]; st->src_port = (uint16_t)w; st->dst_port = (uint16_t)(w >> 16); }
        if ((j = last[(size_t)kIxFlags * stride]) >= 0) st->flags = (uint16_t)((R[(size_t)j * kRecordDwords + 17] >> 16) & A.flags_mask);
        if ((j = last[(size_t)kIxXlatSrcPort * stride]) >= 0) st->xlat_src_port = *reinterpret_cast<const uint16_t*>(A.F.xlat + (size_t)j * kIxXlatBytes + 48);
        if ((j = last[(size_t)kIxXlatDstPort * stride]) >= 0) st->xlat_dst_port = *reinterpret_cast<const uint16_t*>(A.F.xlat + (size_t)j * kIxXlatBytes + 50);
        if ((j = last[(size_t)kIxRtt * stride]) >= 0) st->rtt_ns = *reinterpret_cast<const uint64_t*>(A.F.additional + (size_t)j * kIxAddBytes + 16);
        for (uint32_t k = 0; k < 6; k++) {
            sp[1 + k] = nullptr;
            if ((j = last[(size_t)(kIxStr0 + k) * stride]) >= 0) {
                const IxStrRow& sr = A.srows[A.k8s_rows[2 * (size_t)j + ix_str_side(k)]];
                sp[1 + k] = A.sblob + sr.off[ix_str_field(k)]; sl[1 + k] = sr.len[ix_str_field(k)];
            }
        }
    }
    __syncthreads();
    for (uint32_t k = 0; k < NFAGG_FLP_IPFIX_N_STRINGS; k++) {
        const uint8_t* p = sp[k];
        if (!p) continue;
        const uint32_t n = sl[k];
        for (uint32_t c = threadIdx.x; c < n; c += 256) st->str[k][c] = (char)p[c];
        if (threadIdx.x == 0) st->str_len[k] = n;
    }
}

hipError_t launch_ipfix_flp_plan(const IxArgs& A, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((A.n + kScanBlock - 1) / kScanBlock), stride = blocks + 1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ipfix_carry, dim3(blocks), dim3(kScanBlock), 0, s, A, stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ipfix_carry_scan, dim3(2 * kIxAggs), dim3(kIxScanThreads), 0, s, A.agg, A.pre, blocks, stride);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ipfix_flp_size, dim3(blocks), dim3(kScanBlock), 0, s, A, stride);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_scan_block_sums(A.block_sum, blocks, A.block_base, s)) != hipSuccess) return e;
    return launch_scan_block_sums(A.seq_sum, blocks, A.seq_base, s);
}

hipError_t launch_ipfix_flp_write(const IxArgs& A, uint8_t* d_out, uint64_t* d_msg_offsets, uint8_t* d_status, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((A.n + kScanBlock - 1) / kScanBlock), stride = blocks + 1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ipfix_flp_write, dim3((unsigned)((A.n + 63) / 64)), dim3(64), 0, s, A, d_out, d_msg_offsets, d_status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ipfix_state, dim3(2), dim3(256), 0, s, A, blocks, stride);
    return hipGetLastError();
}

}  // namespace nfagg
