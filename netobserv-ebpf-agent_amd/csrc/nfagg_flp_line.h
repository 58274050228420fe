// nfagg_flp_line.h — the direct-FLP JSON line encoder and the one pair of kernels that runs it: sinks, numbers, addresses,
// MACs, the escaped names, encode_line, the feature-policy contract, k_flp_size<Feat> and k_flp_write<Feat>. nfagg_flp.hip
// instantiates the pair for records that carry only BpfFlowMetrics, nfagg_flp_content.hip for full BpfFlowContents and for
// the lines with TLS names. Device code only.
#pragma once
#include <type_traits>
#include "nfagg_encode.h"
#include "nfagg_flp.h"

namespace nfagg {

// keys, punctuation and numbers of a line with every optional key: 618 bytes; seven directions, names and UDNs on top
constexpr uint32_t kFlpMaxLine = 700 + 7 * (4 + kFlpEscNameMax + 1 + kFlpEscUdnMax + 1);
constexpr uint32_t kFlpWindow = 28672;                       // line starts a window takes, from its aligned base
constexpr uint32_t kFlpLds = kFlpWindow + (kFlpMaxLine + 15) / 16 * 16;
static_assert(kFlpLds <= 32768, "four waves per compute unit");

// kFlpMaxLine counts bytes that no line has: its 700 stands for 618; each of the three lists has one comma fewer than
// entries; TimeFlowEndMs and TimeFlowStartMs have at most 15 characters, not 20 (the seconds of time.Time.Add over two
// int64 nanosecond counts stay within +-1.85e10); Flags is written for protocol 6 alone, whose Proto has one digit, not
// three. kFlpcKeysMax (nfagg_flp_content.hip) counts IPSecRetCode at its longest (27) together with
// "success" (24): the longest pair is the error one, 27 + 22. Without them the maximum is reached.
constexpr uint32_t kFlpLineUnreached = (700 - 618) + 3 + 2 * (20 - 15) + 2, kFlpcLineUnreached = kFlpLineUnreached + 2;

// ---- sinks: CountSink (nfagg_encode.h) only measures, FlpLds writes through a pointer
struct FlpLds {
    uint8_t* p;
    NF_DEV void put(uint8_t b) { *p++ = b; }
};
template <typename S> struct is_count { static constexpr bool value = false; };
template <> struct is_count<CountSink> { static constexpr bool value = true; };

// A literal. Not for the arms of a run-time choice between texts of different lengths (if / else if / else with a lit() each):
// the arms then differ only in constant stores and in the constant added to the sink's pointer, and hipcc 7.2 (clang 22.0.0git)
// was seen to compute the default arm's end pointer under the execution mask of the other lanes. Choose the
// text first and write it with one call (put_text in nfagg_conn_json.hip).
template <typename S, size_t N> NF_DEV void lit(S& s, const char (&a)[N]) {
    if constexpr (is_count<S>::value) s.n += (uint32_t)(N - 1);
    else {
#pragma unroll
        for (size_t k = 0; k + 1 < N; k++) s.put((uint8_t)a[k]);
    }
}

// decimal digits of v < 10^MAXD
template <int MAXD> NF_DEV uint32_t ndigits(uint64_t v) {
    uint32_t nd = 1;
    if constexpr (MAXD <= 10) {
        const uint32_t x = (uint32_t)v;
        uint32_t p = 10;
#pragma unroll
        for (int k = 1; k < MAXD; k++) { nd += x >= p ? 1u : 0u; p *= 10; }
    } else {
        uint64_t p = 10;
#pragma unroll
        for (int k = 1; k < MAXD; k++) { nd += v >= p ? 1u : 0u; p *= 10; }
    }
    return nd;
}

template <int ND> NF_DEV void digits32(uint32_t x, uint8_t* d) {      // ND digits of x, most significant at d[0]
#pragma unroll
    for (int k = ND - 1; k >= 0; k--) { const uint32_t q = x / 10u; d[k] = (uint8_t)(x - q * 10u); x = q; }   // constant divisor: a multiply
}

// strconv-style unsigned decimal. MAXD: the digits the field's type can have (3: uint8, 5: uint16, 10: uint32, 20: uint64).
template <int MAXD, typename S> NF_DEV void dec(S& s, uint64_t v) {
    const uint32_t nd = ndigits<MAXD>(v);
    if constexpr (is_count<S>::value) { s.n += nd; return; }
    else {
        uint8_t d[MAXD];
        if constexpr (MAXD <= 10) digits32<MAXD>((uint32_t)v, d);
        else {                                                         // 2 + 9 + 9 digits; the divisors are constants
            static_assert(MAXD == 20, "uint64");
            const uint64_t hi = v / 1000000000ull;
            const uint32_t lo = (uint32_t)(v - hi * 1000000000ull);
            const uint32_t top = (uint32_t)(hi / 1000000000ull);
            const uint32_t mid = (uint32_t)(hi - (uint64_t)top * 1000000000ull);
            digits32<2>(top, d); digits32<9>(mid, d + 2); digits32<9>(lo, d + 11);
        }
#pragma unroll
        for (int k = 0; k < MAXD; k++)
            if ((uint32_t)k >= (uint32_t)MAXD - nd) s.put((uint8_t)('0' + d[k]));
    }
}
template <typename S> NF_DEV void dec_i64(S& s, int64_t v) {           // strconv.AppendInt(v, 10)
    if (v < 0) { s.put('-'); dec<20>(s, 0ull - (uint64_t)v); } else dec<20>(s, (uint64_t)v);
}

NF_DEV uint8_t hexc(uint32_t x) { return (uint8_t)(x < 10 ? '0' + x : 'a' + (x - 10)); }

// net.HardwareAddr.String(): "%02x" of the six bytes as stored, ':' between them. mac: byte 0 in the low bits.
template <typename S> NF_DEV void mac_text(S& s, uint64_t mac) {
    if constexpr (is_count<S>::value) s.n += 17;
    else {
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const uint32_t b = (uint32_t)(mac >> (8 * k)) & 0xffu;
            if (k) s.put(':');
            s.put(hexc(b >> 4)); s.put(hexc(b & 15));
        }
    }
}

// net.IP.String() of a 16-byte slice: To4() != nil (ten zero bytes, ff ff) prints the dotted quad; otherwise
// netip's appendTo6: the first longest run of at least two zero groups becomes "::", groups in lower-case hex without
// leading zeros.
template <typename S> NF_DEV void ip_text(S& s, const Ip4w& a) {
    if (ip_v4_mapped(a)) {
#pragma unroll
        for (int k = 0; k < 4; k++) { if (k) s.put('.'); dec<3>(s, ip_byte(a, 12 + k)); }
        return;
    }
    uint32_t g[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { const uint32_t h = (a.w[k >> 1] >> (16 * (k & 1))) & 0xffffu; g[k] = ((h & 0xffu) << 8) | (h >> 8); }
    int z0 = -1, zlen = 1, cur = 0, curlen = 0;                        // zlen = 1: only runs of two or more count
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (g[k] == 0) { if (curlen == 0) cur = k; curlen++; if (curlen > zlen) { z0 = cur; zlen = curlen; } }
        else curlen = 0;
    }
    const int z1 = z0 < 0 ? -1 : z0 + zlen;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (k == z0) { s.put(':'); s.put(':'); }
        else if (k < z0 || k >= z1) {
            if (k > 0 && k != z1) s.put(':');
            const uint32_t v = g[k];
            if (v >= 0x1000u) s.put(hexc(v >> 12));
            if (v >= 0x100u) s.put(hexc((v >> 8) & 15));
            if (v >= 0x10u) s.put(hexc((v >> 4) & 15));
            s.put(hexc(v & 15));
        }
    }
}

// An escaped, quoted string of the escaped table: len bytes at p (16-byte aligned), read 16 bytes at a time.
template <typename S> NF_DEV void esc_str(S& s, const uint8_t* p, uint32_t len) {
    if constexpr (is_count<S>::value) s.n += len;
    else {
        for (uint32_t c = 0; c < len; c += 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + c);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (c + k < len) s.put((uint8_t)(w[k >> 2] >> (8 * (k & 3))));
        }
    }
}

NF_DEV bool flp_deferred(const Rec& r) {       // ssl_version @132, tls_cipher_suite @134, tls_key_share @136
    return r.d[33] != 0 || (r.d[34] & 0xffffu) != 0;
}
// What extract conntrack tracks (conntrack.go:70-74): encode_line's `ports` condition and the one k_conn_claim (nfagg_conn.hip)
// applies. Read from the record, never from the id: a tracked flow's total may be 0.
NF_DEV bool conn_tracked(const Rec& r) {
    const uint32_t eth = r.eth(), proto = r.d[9] & 0xffu;
    return (eth == 0x0800u || eth == 0x86DDu) && (proto == 6 || proto == 17 || proto == 132);
}
NF_DEV uint32_t flp_n_intf(const Rec& r) { const uint32_t nb = r.d[24] >> 24; return 1 + (nb > 6 ? 6 : nb); }

// record.go:100-114: the first-seen interface, then the observed ones, all named for (if_index, lMAC), lMAC = dst_mac
// when the first direction is 0 (ingress), src_mac otherwise. row[k]: row of the escaped table (0 = unknown).
NF_DEV void flp_rows(const uint8_t* tab, uint32_t n_names, const Rec& r, uint32_t (&row)[7]) {
    const uint64_t lmac = mac_be((r.d[24] & 0xffu) == 0 ? r.dmac() : r.smac());
    const uint32_t ni = flp_n_intf(r);
#pragma unroll
    for (int k = 0; k < 7; k++) {
        row[k] = 0;
        if ((uint32_t)k < ni) {
            const uint8_t* e = lookup_name(tab, n_names, k == 0 ? r.d[21] : r.d[26 + k], lmac);
            row[k] = e ? (uint32_t)((e - tab) / kNameRowBytes) + 1 : 0u;
        }
    }
}

NF_DEV uint32_t flp_dir(const Rec& r, int k) {   // direction_first_seen @96, observed_direction @100..105
    return k == 0 ? r.d[24] & 0xffu : k <= 4 ? (r.d[25] >> (8 * (k - 1))) & 0xffu : (r.d[26] >> (8 * (k - 5))) & 0xffu;
}

// The keys of a flow's feature parts (DNS, drops, xlat, RTT / IPsec, QUIC, network events) fall in contiguous groups of
// the sorted line; encode_line calls one hook of its feature policy at each. NoFeat: a record that carries only BpfFlowMetrics,
// every hook is empty and the line is the one of decode_protobuf.go:57-127. FlpContent (nfagg_flp_content.hip) holds
// the parts of a full BpfFlowContent, FlpContentNetev adds the flow's resolved network events. The two TLS hooks take the
// record: they are empty in all three, and a record that would need them is deferred; FlpTls (nfagg_tls.h) fills them.
// The three Kubernetes hooks are empty in all of these; FlpK8s (nfagg_k8s.h) fills them. So are the three hooks of the
// transform network rules (FlowDirection, the two subnet labels); kFlagNames = false keeps dec<5> as the value of Flags, and no
// call stands in its place. FlpNet (nfagg_net.h) fills the hooks and names the flags. The last hook, in front of the closing
// brace, takes the two keys extract conntrack adds to a flow log; FlpConnMeta (nfagg_conn_meta.h) fills it. Every layer runs in
// the one kernel pair below: an instantiation per policy, so that each keeps its own code and registers.
//
// What k_flp_size<Feat> and k_flp_write<Feat> ask of a policy beside the hooks, all of it known when they are compiled:
//   kWindow   line starts a window of the write kernel takes, from its 16-byte aligned base
//   kLds      the window's LDS: kWindow plus the longest line, rounded up to 16
//   kSideLds  the LDS a wave holds beside the window: 64 x 32 for a DNS name slot per lane; 0 or 16 for none
//   kDefers   a record with TLS names (flp_deferred) gets no line, is flagged and counted; false: the policy has a member
//             `tls` that takes the kernel's TLS name table, and the record is written
//   kMaxLine  the longest line the policy reaches; FlpTls sizes its window from it
//   load(F, i, slot)   reads record i's feature parts, only for a line that is measured or written
//   kJoins    the policy has load_joins(J, i), which reads what its layers join to record i (FlpK8s the Kubernetes rows, FlpNet
//             the net row as well, FlpConnMeta the hash id too); false: no call is compiled
//   kTrackedOnly   a flow extract conntrack does not track (conn_tracked) gets a zero-length line and is never encoded
//             (FlpConnMeta); false: no guard is compiled (one compiled for every policy cost the TLS write kernels 0.4-0.6 %,
//             profiles/flp_one_kernel_pair_ab.txt)
// A policy without data members (FlpPlain) is not asked to load: handing the kernel's F to an empty function by reference is
// enough to change the register allocation of k_flp_write<FlpPlain> (530 instructions more). The table is
// assigned, not handed to a setter, for the same reason.
struct NoFeat {
    template <typename S> NF_DEV void dns(S&) const {}        // Dns*          after Bytes
    template <typename S> NF_DEV void ipsec(S&) const {}      // IPSec*        after Flags
    template <typename S> NF_DEV void netev(S&) const {}      // NetworkEvents after Interfaces
    template <typename S> NF_DEV void drops(S&) const {}      // PktDrop*      after Packets
    template <typename S> NF_DEV void quic(S&) const {}       // Quic*         after Proto
    template <typename S> NF_DEV void rtt(S&) const {}        // TimeFlowRttNs after TimeFlowEndMs
    template <typename S> NF_DEV void xlat(S&) const {}       // Xlat*         after Udns
    template <typename S> NF_DEV void zone(S&) const {}       // ZoneId        last
    template <typename S> NF_DEV void tls_names(S&, const Rec&) const {}     // TLSCipherSuite TLSGroup  after SrcPort
    template <typename S> NF_DEV void tls_version(S&, const Rec&) const {}   // TLSVersion               after TLSTypes
    template <typename S> NF_DEV void k8s_dst(S&) const {}    // DstK8S_*      after DstAddr
    template <typename S> NF_DEV void k8s_layer(S&) const {}  // K8S_FlowLayer after Interfaces, before NetworkEvents
    template <typename S> NF_DEV void k8s_src(S&) const {}    // SrcK8S_*      after SrcAddr
    static constexpr bool kFlagNames = false;                 // true: flags_value(s, flags) writes the value of Flags
    template <typename S> NF_DEV void dst_subnet(S&) const {}      // DstSubnetLabel after DstPort
    template <typename S> NF_DEV void flow_direction(S&) const {}  // FlowDirection  after Flags
    template <typename S> NF_DEV void src_subnet(S&) const {}      // SrcSubnetLabel after SrcPort
    template <typename S> NF_DEV void conn_meta(S&) const {}       // _HashId _RecordType  behind ZoneId: '_' sorts above every letter a key starts with
    static constexpr bool kJoins = false, kTrackedOnly = false;
};
// The plain policy: the line of the records Accounter.evict produces.
struct FlpPlain : NoFeat {
    static constexpr uint32_t kWindow = kFlpWindow, kLds = kFlpLds, kSideLds = 0, kMaxLine = kFlpMaxLine - kFlpLineUnreached;
    static constexpr bool kDefers = true;
    NF_DEV void load(const PbFeat&, uint64_t, uint8_t*) {}       // for FlpTls<FlpPlain>, which is not empty
};

// One line. Same code measures (CountSink) and writes (FlpLds). The policy travels by value: a reference to an empty policy
// is enough to change the register allocation of k_flp_write<FlpPlain>.
template <typename S, typename F>
NF_DEV void encode_line(S& s, const Rec& r, const FlpParams& P, const uint32_t (&row)[7], F f) {
    const uint32_t eth = r.eth(), proto = r.d[9] & 0xffu;
    const bool ip = eth == 0x0800u || eth == 0x86DDu;
    const bool icmp = ip && (proto == 1 || proto == 58), ports = ip && (proto == 6 || proto == 17 || proto == 132);
    const uint32_t ni = flp_n_intf(r);
    lit(s, "{\"AgentIP\":\"");
    if (P.agent_nil) lit(s, "<nil>");
    else ip_text(s, Ip4w{{P.agent_ip_w[0], P.agent_ip_w[1], P.agent_ip_w[2], P.agent_ip_w[3]}});
    s.put('"');
    if (r.bytes()) { lit(s, ",\"Bytes\":"); dec<20>(s, r.bytes()); }
    f.dns(s);
    if (ip) {
        lit(s, ",\"Dscp\":"); dec<3>(s, r.dscp());
        lit(s, ",\"DstAddr\":\""); ip_text(s, Ip4w{{r.d[4], r.d[5], r.d[6], r.d[7]}}); s.put('"');
        f.k8s_dst(s);
    }
    lit(s, ",\"DstMac\":\""); mac_text(s, r.dmac()); s.put('"');
    if (ports) { lit(s, ",\"DstPort\":"); dec<5>(s, r.d[8] >> 16); }
    f.dst_subnet(s);
    lit(s, ",\"Etype\":"); dec<5>(s, eth);
    if (ip && proto == 6) {
        lit(s, ",\"Flags\":");
        if constexpr (F::kFlagNames) f.flags_value(s, r.flags()); else dec<5>(s, r.flags());
    }
    f.flow_direction(s);
    f.ipsec(s);
    if (icmp) {
        lit(s, ",\"IcmpCode\":"); dec<3>(s, (r.d[9] >> 16) & 0xffu);
        lit(s, ",\"IcmpType\":"); dec<3>(s, (r.d[9] >> 8) & 0xffu);
    }
    lit(s, ",\"IfDirections\":[");
#pragma unroll
    for (int k = 0; k < 7; k++)
        if ((uint32_t)k < ni) { if (k) s.put(','); dec<3>(s, flp_dir(r, k)); }
    lit(s, "],\"Interfaces\":[");
    uint32_t lens[7] = {};
#pragma unroll
    for (int k = 0; k < 7; k++)
        if ((uint32_t)k < ni) {
            const uint8_t* e = P.esc + (size_t)row[k] * kFlpEscRowBytes;
            lens[k] = *reinterpret_cast<const uint32_t*>(e);           // name_len | udn_len << 16
            if (k) s.put(',');
            esc_str(s, e + kFlpEscNameOff, lens[k] & 0xffffu);
        }
    s.put(']');
    f.k8s_layer(s);
    f.netev(s);
    if (r.packets()) { lit(s, ",\"Packets\":"); dec<10>(s, r.packets()); }
    f.drops(s);
    if (ip) { lit(s, ",\"Proto\":"); dec<3>(s, proto); }
    f.quic(s);
    if (r.sampling()) { lit(s, ",\"Sampling\":"); dec<10>(s, r.sampling()); }
    if (ip) { lit(s, ",\"SrcAddr\":\""); ip_text(s, Ip4w{{r.d[0], r.d[1], r.d[2], r.d[3]}}); s.put('"'); f.k8s_src(s); }
    lit(s, ",\"SrcMac\":\""); mac_text(s, r.smac()); s.put('"');
    if (ports) { lit(s, ",\"SrcPort\":"); dec<5>(s, r.d[8] & 0xffffu); }
    f.src_subnet(s);
    f.tls_names(s, r);
    const uint32_t tls = (r.d[34] >> 16) & 0xffu;                      // tls_types @138
    if (tls) {   // tlsTypesToStrings (pkg/model/tls_types.go) in its order; no known bit: a nil slice, "null"
        lit(s, ",\"TLSTypes\":");
        if ((tls & 63u) == 0) lit(s, "null");
        else {
            s.put('[');
            bool first = true;
            if (tls & 1u) { lit(s, "\"ClientHello\""); first = false; }
            if (tls & 2u) { if (!first) s.put(','); lit(s, "\"ServerHello\""); first = false; }
            if (tls & 4u) { if (!first) s.put(','); lit(s, "\"OtherHandshake\""); first = false; }
            if (tls & 8u) { if (!first) s.put(','); lit(s, "\"ChangeCipher\""); first = false; }
            if (tls & 16u) { if (!first) s.put(','); lit(s, "\"Alert\""); first = false; }
            if (tls & 32u) { if (!first) s.put(','); lit(s, "\"AppData\""); }
            s.put(']');
        }
    }
    f.tls_version(s, r);
    const TimeParts ts = flow_time(P.now_sec, P.now_nsec, P.mono_now, r.start());
    const TimeParts te = flow_time(P.now_sec, P.now_nsec, P.mono_now, r.end());
    lit(s, ",\"TimeFlowEndMs\":"); dec_i64(s, te.sec * 1000 + te.nsec / 1000000);      // t.UnixMilli()
    f.rtt(s);
    lit(s, ",\"TimeFlowStartMs\":"); dec_i64(s, ts.sec * 1000 + ts.nsec / 1000000);
    lit(s, ",\"TimeReceived\":"); dec_i64(s, P.time_received);
    lit(s, ",\"Udns\":[");
#pragma unroll
    for (int k = 0; k < 7; k++)
        if ((uint32_t)k < ni) {
            if (k) s.put(',');
            esc_str(s, P.esc + (size_t)row[k] * kFlpEscRowBytes + kFlpEscUdnOff, lens[k] >> 16);
        }
    s.put(']');
    f.xlat(s);
    f.zone(s);
    f.conn_meta(s);
    lit(s, "}\n");
}

// What the layers above FlpTls join to a record: FlpLineArgs' last five members, as load_joins and the kernels take them. The
// kernels keep the arguments every policy reads where they were and take the joins as one struct behind them, so the twelve
// kernels below FlpK8s read their arguments at the offsets they had. Taking FlpLineArgs whole moved every size kernel's scalar
// spills; so did the five members as arguments of their own, which also moved four write kernels' scratch
// (profiles/flp_line_args_codeobj.txt).
struct FlpJoins { K8sDev K; NetDev N; const uint32_t* k8s_rows; const uint2* net_rows; const uint64_t* hash_ids; };

// ---- kernel 1: line length per record (the seven interface rows resolved once), block-local exclusive scan. rows: 8 dwords
// per record, rows 0..6 and the length (0: deferred, or a flow extract conntrack does not track, whose rows stay 0 as well).
template <typename Feat>
__global__ __launch_bounds__(kScanBlock) void k_flp_size(const void* __restrict__ recs, uint64_t n, FlpParams P, PbFeat F, TlsDev T,
                                                         uint32_t* __restrict__ rows, uint32_t* __restrict__ local_off,
                                                         uint32_t* __restrict__ block_sum, uint32_t* __restrict__ n_deferred, FlpJoins J) {
    constexpr uint32_t kSlot = Feat::kSideLds >= 64 * 32 ? 32 : 0;       // a DNS name slot per lane where the policy reads one
    constexpr bool kHolds = !std::is_empty_v<Feat>;                      // the policy has members to fill
    __shared__ uint32_t wave_tot[kScanBlock / 64];
    __shared__ __align__(16) uint8_t name_lds[kSlot ? kScanBlock * kSlot : 16];
    __shared__ uint32_t tab_lds[kNamesLdsRows * (kNameRowBytes / 4)];
    const uint8_t* tab = stage_names<kScanBlock>(P.names, P.n_names, tab_lds);
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t len = 0;
    bool deferred = false;
    if (i < n) {
        Rec r;
        load_record(recs, i, r);
        uint32_t row[7] = {};
        bool line = true;
        if constexpr (Feat::kTrackedOnly) line = conn_tracked(r); else flp_rows(tab, P.n_names, r, row);
        if constexpr (Feat::kDefers) { deferred = flp_deferred(r); line = !deferred; }
        if (line) {
            if constexpr (Feat::kTrackedOnly) flp_rows(tab, P.n_names, r, row);
            Feat f;
            if constexpr (kHolds) f.load(F, i, name_lds + threadIdx.x * kSlot);
            if constexpr (!Feat::kDefers) f.tls = T;
            if constexpr (Feat::kJoins) f.load_joins(J, i);
            CountSink c;
            encode_line(c, r, P, row, f);
            len = c.n;
        }
        uint4* o = reinterpret_cast<uint4*>(rows + i * 8);
        o[0] = make_uint4(row[0], row[1], row[2], row[3]);
        o[1] = make_uint4(row[4], row[5], row[6], len);
    }
    if constexpr (Feat::kDefers) {
        const int lane = threadIdx.x & 63;
        const uint64_t dm = __ballot(deferred);
        if (lane == 0 && dm) atomicAdd(n_deferred, (uint32_t)__popcll(dm));
    }
    block_scan(len, i, n, wave_tot, local_off, block_sum);
}

// ---- kernel 3: write. One wave per 64 consecutive records; their lines are contiguous in the output. The wave moves a
// window along its byte range [shift, span) of the image: a window starts at a line start `lo`, takes every line that
// starts less than Feat::kWindow bytes behind its 16-byte aligned base, and ends where the last of them ends, so a line is
// always written whole (the buffer has the longest line's bytes of slack) and exactly once. A lane without a line (deferred,
// not tracked) is passed over.
template <typename Feat>
__global__ __launch_bounds__(64) void k_flp_write(const void* __restrict__ recs, uint64_t n, FlpParams P, PbFeat F, TlsDev T,
                                                  const uint32_t* __restrict__ rows, const uint32_t* __restrict__ local_off,
                                                  const uint64_t* __restrict__ block_base, uint8_t* __restrict__ out,
                                                  uint64_t* __restrict__ line_offsets, uint8_t* __restrict__ deferred, FlpJoins J) {
    constexpr uint32_t kSlot = Feat::kSideLds >= 64 * 32 ? 32 : 0;
    constexpr bool kHolds = !std::is_empty_v<Feat>;
    constexpr bool kSkips = Feat::kDefers || Feat::kTrackedOnly;         // a record without a line: its parts and rows are not read
    static_assert(Feat::kLds + Feat::kSideLds <= 32768, "four waves per compute unit");
    __shared__ __align__(16) uint8_t lds[Feat::kLds];
    __shared__ __align__(16) uint8_t name_lds[kSlot ? 64 * kSlot : 16];
    const uint64_t i0 = (uint64_t)blockIdx.x * 64, i = i0 + threadIdx.x;
    WaveImage w(block_base, local_off, i0);
    uint64_t my_off = 0; uint32_t my_len = 0;
    uint32_t row[7] = {};
    Rec r;
    Feat f;
    if constexpr (!Feat::kDefers) f.tls = T;
    if (i < n) {
        load_record(recs, i, r);
        const uint4* q = reinterpret_cast<const uint4*>(rows + i * 8);
        const uint4 a = q[0], b = q[1];
        row[0] = a.x; row[1] = a.y; row[2] = a.z; row[3] = a.w; row[4] = b.x; row[5] = b.y; row[6] = b.z;
        my_len = b.w;                                                 // every line that is written has at least its braces
        if constexpr (kHolds) {
            if (!kSkips || my_len) {
                f.load(F, i, name_lds + threadIdx.x * kSlot);
                if constexpr (Feat::kJoins) f.load_joins(J, i);
            }
        }
        my_off = record_off(block_base, local_off, i);
        line_offsets[i] = my_off;
        if (i == n - 1) line_offsets[n] = my_off + my_len;
        if constexpr (Feat::kDefers) { if (deferred) deferred[i] = my_len == 0 ? 1 : 0; }
    }
    w.close(my_off + my_len, out);
    const uint32_t p0 = w.pos(my_off);                            // my line = image bytes [p0, p0 + my_len)
    uint32_t lo = w.shift;
    while (lo < w.span) {
        const uint32_t base = lo & ~15u;
        const bool mine = my_len && p0 >= lo && p0 - base < Feat::kWindow;
        if (mine) { FlpLds s{lds + (p0 - base)}; encode_line(s, r, P, row, f); }
        uint32_t hi = mine ? p0 + my_len : lo;                  // the window's end: at most base + the window + the longest line
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(hi, d, 64); hi = o > hi ? o : hi; }
        __syncthreads();
        copy_image_out(w.dst, lds, base, lo, hi);
        __syncthreads();
        lo = hi;
    }
}

// The two launches for one policy. Each instantiation lives in one translation unit: the plain one in nfagg_flp.hip (declared
// below, so that no other file compiles it), the others in nfagg_flp_content.hip, where launch_flp_size / launch_flp_write select.
template <typename Feat>
__attribute__((noinline)) hipError_t flp_size_as(const FlpLineArgs& A, uint32_t* d_rows, uint32_t* d_local_off, uint32_t* d_block_sum,
                                                 uint64_t* d_block_base, uint32_t* d_n_deferred, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((A.n + kScanBlock - 1) / kScanBlock);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_flp_size<Feat>, dim3(blocks), dim3(kScanBlock), 0, s, A.recs, A.n, A.P, A.F, A.T, d_rows, d_local_off, d_block_sum,
                       d_n_deferred, FlpJoins{A.K, A.N, A.k8s_rows, A.net_rows, A.hash_ids});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_block_sums(d_block_sum, blocks, d_block_base, s);
}
template <typename Feat>
__attribute__((noinline)) hipError_t flp_write_as(const FlpLineArgs& A, const uint32_t* d_rows, const uint32_t* d_local_off,
                                                  const uint64_t* d_block_base, void* d_out, uint64_t* d_line_offsets, uint8_t* d_deferred,
                                                  hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_flp_write<Feat>, dim3((unsigned)((A.n + 63) / 64)), dim3(64), 0, s, A.recs, A.n, A.P, A.F, A.T, d_rows, d_local_off,
                       d_block_base, (uint8_t*)d_out, d_line_offsets, d_deferred, FlpJoins{A.K, A.N, A.k8s_rows, A.net_rows, A.hash_ids});
    return hipGetLastError();
}
extern template hipError_t flp_size_as<FlpPlain>(const FlpLineArgs&, uint32_t*, uint32_t*, uint32_t*, uint64_t*, uint32_t*, hipStream_t);
extern template hipError_t flp_write_as<FlpPlain>(const FlpLineArgs&, const uint32_t*, const uint32_t*, const uint64_t*, void*, uint64_t*,
                                                  uint8_t*, hipStream_t);

}  // namespace nfagg
