// nfagg_flp_line.h — the direct-FLP JSON line encoder the two pairs of kernels share (nfagg_flp.hip: records that carry
// only BpfFlowMetrics; nfagg_flp_content.hip: full BpfFlowContents): sinks, numbers, addresses, MACs, the escaped names,
// and encode_line itself. Device code only.
#pragma once
#include "nfagg_encode.h"
#include "nfagg_flp.h"

namespace nfagg {

// keys, punctuation and numbers of a line with every optional key: 618 bytes; seven directions, names and UDNs on top
constexpr uint32_t kFlpMaxLine = 700 + 7 * (4 + kFlpEscNameMax + 1 + kFlpEscUdnMax + 1);

// ---- sinks: CountSink (nfagg_encode.h) only measures, FlpLds writes through a pointer
struct FlpLds {
    uint8_t* p;
    NF_DEV void put(uint8_t b) { *p++ = b; }
};
template <typename S> struct is_count { static constexpr bool value = false; };
template <> struct is_count<CountSink> { static constexpr bool value = true; };

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
    if ((a.w[0] | a.w[1]) == 0 && a.w[2] == 0xffff0000u) {
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

// The keys of a flow's feature parts (DNS, drops, xlat, RTT / IPsec, QUIC, network events) fall in ten contiguous groups of
// the sorted line; encode_line calls one hook of its feature policy at each. NoFeat: a record that carries only BpfFlowMetrics,
// every hook is empty and the line is the one of decode_protobuf.go:57-127. FlpContent (nfagg_flp_content.hip) holds
// the parts of a full BpfFlowContent, FlpContentNetev adds the flow's resolved network events. The two TLS hooks take the
// record: they are empty in all three, and a record that would need them is deferred; FlpTls (nfagg_tls.h) fills them.
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
};

// One line. Same code measures (CountSink) and writes (FlpLds). The policy travels by value: a reference to an empty NoFeat
// is enough to change the register allocation of k_flp_write.
template <typename S, typename F = NoFeat>
NF_DEV void encode_line(S& s, const Rec& r, const FlpParams& P, const uint32_t (&row)[7], F f = F{}) {
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
    }
    lit(s, ",\"DstMac\":\""); mac_text(s, r.dmac()); s.put('"');
    if (ports) { lit(s, ",\"DstPort\":"); dec<5>(s, r.d[8] >> 16); }
    lit(s, ",\"Etype\":"); dec<5>(s, eth);
    if (ip && proto == 6) { lit(s, ",\"Flags\":"); dec<5>(s, r.flags()); }
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
    f.netev(s);
    if (r.packets()) { lit(s, ",\"Packets\":"); dec<10>(s, r.packets()); }
    f.drops(s);
    if (ip) { lit(s, ",\"Proto\":"); dec<3>(s, proto); }
    f.quic(s);
    if (r.sampling()) { lit(s, ",\"Sampling\":"); dec<10>(s, r.sampling()); }
    if (ip) { lit(s, ",\"SrcAddr\":\""); ip_text(s, Ip4w{{r.d[0], r.d[1], r.d[2], r.d[3]}}); s.put('"'); }
    lit(s, ",\"SrcMac\":\""); mac_text(s, r.smac()); s.put('"');
    if (ports) { lit(s, ",\"SrcPort\":"); dec<5>(s, r.d[8] & 0xffffu); }
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
    lit(s, "}\n");
}

}  // namespace nfagg
