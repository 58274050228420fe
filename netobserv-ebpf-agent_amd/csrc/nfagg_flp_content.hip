// nfagg_flp_content.hip — MapTracer flows (pkg/flow/tracer_map.go:103-146: a flow_record_t plus the feature parts of a
// full model.BpfFlowContent) -> direct-FLP JSON lines. The line of nfagg_flp.hip with the keys that
//   pkg/decode/decode_protobuf.go:130-192   RecordToMap, the feature parts
//   pkg/model/record.go:116-125             NewRecord: DNSLatency, TimeFlowRtt
// add, at their places in byte order ([] = only when RecordToMap's rule says so):
//   after Bytes:         [DnsErrno] [DnsFlags DnsFlagsResponseCode DnsId DnsLatencyMs [DnsName]]
//   after Flags:         [IPSecRetCode IPSecStatus]
//   after Packets:       [PktDropBytes PktDropLatestDropCause PktDropLatestFlags PktDropLatestState PktDropPackets]
//   after Proto:         [QuicSeenLongHdr QuicSeenShortHdr QuicVersion]
//   after TimeFlowEndMs: [TimeFlowRttNs]
//   after Udns:          [XlatDstAddr [XlatDstPort] XlatSrcAddr [XlatSrcPort]] [ZoneId]
//   after Interfaces:    [NetworkEvents]      (decode_protobuf.go:184-186; the *_netev entry points only)
// Without a cookie table network events are encoded as NewRecord does with a nil decoder (record.go:126): no key, no drop
// injected. With one (FlpContentNetev) the line carries the rendered objects of the rows nfagg_netev_resolve found; the
// drop it injected arrives in the drops part like any other.
//
// Same two passes, same window scheme, same encode_line and the same two kernels as nfagg_flp.hip (k_flp_size<Feat>,
// k_flp_write<Feat> of nfagg_flp_line.h), with FlpContent as the feature policy: this file compiles them for FlpContent and
// FlpContentNetev, for FlpTls (nfagg_tls.h), FlpK8s (nfagg_k8s.h), FlpNet (nfagg_net.h) and FlpConnMeta (nfagg_conn_meta.h)
// layered over those two and over FlpPlain, and selects among all fifteen. A lane reads the parts its
// present byte names with 16- and 8-byte loads before anything is emitted, keeps the fields the line needs in registers
// and the DNS name in a 32-byte LDS slot of its own. The names of response codes, TCP states and drop causes sit in one
// constant blob with an offset and a length per name; the counting pass reads only the lengths.
#include "nfagg_flp_line.h"
#include "nfagg_flp_names.h"
#include "nfagg_netev.h"
#include "nfagg_tls.h"
#include "nfagg_k8s.h"
#include "nfagg_net.h"
#include "nfagg_conn_meta.h"
#include "nfagg_loki_line.h"

namespace nfagg {

constexpr uint32_t cstr_len(const char* p) { uint32_t n = 0; while (p[n]) n++; return n; }
constexpr uint32_t flp_names_dwords() {
    uint32_t d = 0;
    for (uint32_t k = 0; k < kFlpNameCount; k++) d += (cstr_len(kFlpNames[k]) + 3) / 4;
    return d;
}
constexpr uint32_t flp_names_longest() {
    uint32_t m = 0;
    for (uint32_t k = 0; k < kFlpNameCount; k++) m = cstr_len(kFlpNames[k]) > m ? cstr_len(kFlpNames[k]) : m;
    return m;
}
// Each name starts at a dword of the blob: a name is read four bytes at a time.
struct FlpNameTab {
    uint8_t len[kFlpNameCount];
    uint16_t off[kFlpNameCount];                 // in dwords
    uint32_t blob[flp_names_dwords()];
};
constexpr FlpNameTab make_flp_names() {
    FlpNameTab t{};
    uint32_t o = 0;
    for (uint32_t k = 0; k < kFlpNameCount; k++) {
        const uint32_t n = cstr_len(kFlpNames[k]);
        for (uint32_t b = 0; b < n; b++) t.blob[o + b / 4] |= (uint32_t)(uint8_t)kFlpNames[k][b] << (8 * (b & 3));
        t.len[k] = (uint8_t)n; t.off[k] = (uint16_t)o;
        o += (n + 3) / 4;
    }
    return t;
}
__constant__ FlpNameTab d_flp_names = make_flp_names();

// "name" of the table, quotes included. No name needs escaping.
template <typename S> NF_DEV void table_str(S& s, uint32_t idx) {
    const uint32_t len = d_flp_names.len[idx];
    if constexpr (is_count<S>::value) s.n += len + 2;
    else {
        const uint32_t* p = d_flp_names.blob + d_flp_names.off[idx];
        s.put('"');
        for (uint32_t c = 0; c < len; c += 4) {
            const uint32_t w = p[c >> 2];
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (c + k < len) s.put((uint8_t)(w >> (8 * k)));
        }
        s.put('"');
    }
}

// jsoniter's WriteString escaping (stream_str.go:311-372, as flp_escape of nfagg_api_tables.hip does for the namer table), one
// byte at a time in front of another sink: the DNS name is the one string of a line that the host has not seen.
template <typename S> struct EscSink {
    S& s;
    NF_DEV void put(uint8_t b) {
        if (b > 31 && b != '"' && b != '\\') { s.put(b); return; }
        s.put('\\');
        if (b == '"' || b == '\\') s.put(b);
        else if (b == '\n') s.put('n');
        else if (b == '\r') s.put('r');
        else if (b == '\t') s.put('t');
        else { s.put('u'); s.put('0'); s.put('0'); s.put(hexc(b >> 4)); s.put(hexc(b & 15)); }
    }
};

// model.AllZeroIP (record.go:233-238): net.IPv6zero, or net.IPv4zero in its 16-byte form ::ffff:0.0.0.0

// The longest line: every key of nfagg_flp.hip's worst case plus, in the order of the list above, 15 + 17 + 35 + 14 + 30
// + 11 + (2 + 6 x 31: a dotted name has at most 31 bytes) for DNS, 27 + 24 for IPsec, 21 + (28 + the longest name) + 27
// + 41 + 23 for drops, 22 + 23 + 42 for QUIC, 37 for the RTT, 2 x 56 + 2 x 20 + 15 for xlat and the zone.
constexpr uint32_t kFlpcKeysMax = (15 + 17 + 35 + 14 + 30 + 11 + 2 + 6 * 31) + (27 + 24) + (21 + 28 + flp_names_longest() + 27 + 41 + 23) +
                                  (22 + 23 + 42) + 37 + (2 * 56 + 2 * 20 + 15);
constexpr uint32_t kFlpcMaxLine = kFlpMaxLine + kFlpcKeysMax;
constexpr uint32_t kFlpcNameLds = 64 * 32;                    // the wave's DNS name slots
constexpr uint32_t kFlpcWindow = 25600;                       // line starts a window takes, from its aligned base
constexpr uint32_t kFlpcLds = kFlpcWindow + (kFlpcMaxLine + 15) / 16 * 16;
static_assert(kFlpcLds + kFlpcNameLds <= 32768, "four waves per compute unit");

// With network events the longest line grows by the key, four rendered objects at their cap, the commas between them
// and the closing bracket; the window shrinks by as much, so that the wave's LDS stays at 32 KiB.
constexpr uint32_t kFlpnMaxLine = kFlpcMaxLine + (sizeof(",\"NetworkEvents\":[") - 1) + 4 * kNetevMaxRendered + 3 + 1;
constexpr uint32_t kFlpnWindow = (32768 - kFlpcNameLds - (kFlpnMaxLine + 15) / 16 * 16) / 16 * 16;
constexpr uint32_t kFlpnLds = kFlpnWindow + (kFlpnMaxLine + 15) / 16 * 16;
static_assert(kFlpnLds + kFlpcNameLds <= 32768 && kFlpnWindow >= 16384, "four waves per compute unit, and a window worth its copy-out");

// The feature parts of one flow, as encode_line's feature policy. load() reads the parts that are present (array given
// and the flow's present byte has the bit) and nothing of the others.
struct FlpContent {
    static constexpr uint32_t kWindow = kFlpcWindow, kLds = kFlpcLds, kSideLds = kFlpcNameLds, kMaxLine = kFlpcMaxLine - kFlpcLineUnreached;
    static constexpr bool kDefers = true, kJoins = false, kTrackedOnly = false;
    uint32_t have = 0;          // NFAGG_FEAT_* bits of the parts that were loaded
    uint32_t add[4] = {};       // additional_metrics @16: flow_rtt (2), ipsec_encrypted_ret, eth | ipsec_encrypted << 16
    uint32_t dnsw[4] = {};      // dns_metrics @16: latency (2), id | flags << 16, eth | errno << 16 | name[0] << 24
    uint32_t drp[4] = {};       // pkt_drop_metrics @16: bytes | packets << 16, cause, flags | eth << 16, state
    uint32_t xlt[10] = {};      // xlat_metrics @16: saddr (4), daddr (4), sport | dport << 16, zone | eth << 16
    uint32_t quc[2] = {};       // quic_metrics @16: version, eth | long << 16 | short << 24
    const uint8_t* name = nullptr;   // dns_metrics.name, 32 bytes in this lane's LDS slot (16-byte aligned)

    NF_DEV void load(const PbFeat& F, uint64_t i, uint8_t* name_lds) {
        const uint32_t p = F.present ? F.present[i] : 0u;
        have = (F.additional ? p & NFAGG_FEAT_ADDITIONAL : 0u) | (F.dns ? p & NFAGG_FEAT_DNS : 0u) | (F.drops ? p & NFAGG_FEAT_DROPS : 0u) |
               (F.xlat ? p & NFAGG_FEAT_XLAT : 0u) | (F.quic ? p & NFAGG_FEAT_QUIC : 0u);
        name = name_lds;
        if (have & NFAGG_FEAT_ADDITIONAL) {
            uint32_t w[8]; load_dwords16(F.additional + i * 32, w);
#pragma unroll
            for (int k = 0; k < 4; k++) add[k] = w[4 + k];
        }
        if (have & NFAGG_FEAT_DNS) {     // name @31..62 is unaligned: whole struct in, the name out of the registers
            uint32_t w[16]; load_dwords16(F.dns + i * 64, w);
#pragma unroll
            for (int k = 0; k < 4; k++) dnsw[k] = w[4 + k];
            uint32_t nm[8];
#pragma unroll
            for (int k = 0; k < 8; k++) nm[k] = (w[7 + k] >> 24) | (w[8 + k] << 8);
            uint4* slot = reinterpret_cast<uint4*>(name_lds);
            slot[0] = make_uint4(nm[0], nm[1], nm[2], nm[3]); slot[1] = make_uint4(nm[4], nm[5], nm[6], nm[7]);
        }
        if (have & NFAGG_FEAT_DROPS) {
            uint32_t w[8]; load_dwords16(F.drops + i * 32, w);
#pragma unroll
            for (int k = 0; k < 4; k++) drp[k] = w[4 + k];
        }
        if (have & NFAGG_FEAT_XLAT) {
            uint32_t w[14]; load_dwords8(F.xlat + i * 56, w);
#pragma unroll
            for (int k = 0; k < 10; k++) xlt[k] = w[4 + k];
        }
        if (have & NFAGG_FEAT_QUIC) {
            uint32_t w[6]; load_dwords8(F.quic + i * 24, w);
            quc[0] = w[4]; quc[1] = w[5];
        }
    }

    template <typename S> NF_DEV void dns(S& s) const {                 // decode_protobuf.go:130-143
        if (!(have & NFAGG_FEAT_DNS)) return;
        const uint32_t err = (dnsw[3] >> 16) & 0xffu, id = dnsw[2] & 0xffffu, flags = dnsw[2] >> 16;
        if (err) { lit(s, ",\"DnsErrno\":"); dec<3>(s, err); }
        if (!id) return;
        lit(s, ",\"DnsFlags\":"); dec<5>(s, flags);
        const uint32_t rc = flags & 15u;
        lit(s, ",\"DnsFlagsResponseCode\":"); table_str(s, rcode_name(rc));
        lit(s, ",\"DnsId\":"); dec<5>(s, id);
        // record.go:116-120 + Duration.Milliseconds(): int64(latency) / 1e6, truncating towards zero
        lit(s, ",\"DnsLatencyMs\":"); dec_i64(s, (int64_t)((uint64_t)dnsw[0] | ((uint64_t)dnsw[1] << 32)) / 1000000ll);
        CountSink c;
        if (dns_dotted<false>(c, name)) {
            lit(s, ",\"DnsName\":\"");
            EscSink<S> e{s};
            dns_dotted<true>(e, name);
            s.put('"');
        }
    }
    template <typename S> NF_DEV void ipsec(S& s) const {               // decode_protobuf.go:170-178
        if (!(have & NFAGG_FEAT_ADDITIONAL)) return;
        const int32_t ret = (int32_t)add[2];
        if (ret != 0) { lit(s, ",\"IPSecRetCode\":"); dec_i64(s, ret); lit(s, ",\"IPSecStatus\":\"error\""); }
        else if ((add[3] >> 16) & 0xffu) lit(s, ",\"IPSecRetCode\":0,\"IPSecStatus\":\"success\"");
    }
    template <typename S> NF_DEV void netev(S&) const {}                // record.go:126 with a nil decoder; FlpContentNetev has the key
    template <typename S> NF_DEV void drops(S& s) const {               // decode_protobuf.go:145-153
        if (!(have & NFAGG_FEAT_DROPS) || drp[1] == 0) return;
        lit(s, ",\"PktDropBytes\":"); dec<5>(s, drp[0] & 0xffffu);
        lit(s, ",\"PktDropLatestDropCause\":"); table_str(s, drop_cause_name(drp[1]));
        lit(s, ",\"PktDropLatestFlags\":"); dec<5>(s, drp[2] & 0xffffu);
        const uint32_t st = drp[3] & 0xffu;
        lit(s, ",\"PktDropLatestState\":"); table_str(s, tcp_state_name(st));
        lit(s, ",\"PktDropPackets\":"); dec<5>(s, drp[0] >> 16);
    }
    template <typename S> NF_DEV void quic(S& s) const {                // decode_protobuf.go:188-192, record.go:259-270
        if (!(have & NFAGG_FEAT_QUIC)) return;
        lit(s, ",\"QuicSeenLongHdr\":"); dec<3>(s, (quc[1] >> 16) & 0xffu);
        lit(s, ",\"QuicSeenShortHdr\":"); dec<3>(s, quc[1] >> 24);
        lit(s, ",\"QuicVersion\":\"QUIC ");
        if (quc[0] <= 1) { s.put('v'); s.put((uint8_t)('1' + quc[0])); }
        else { lit(s, "Unknown ("); dec<10>(s, quc[0]); s.put(')'); }
        s.put('"');
    }
    template <typename S> NF_DEV void rtt(S& s) const {                 // record.go:121-125, decode_protobuf.go:180-182
        const uint64_t v = (uint64_t)add[0] | ((uint64_t)add[1] << 32);
        if ((have & NFAGG_FEAT_ADDITIONAL) && v) { lit(s, ",\"TimeFlowRttNs\":"); dec_i64(s, (int64_t)v); }
    }
    NF_DEV bool xlated() const {                                        // decode_protobuf.go:155-157
        return (have & NFAGG_FEAT_XLAT) && !ip_all_zero(Ip4w{{xlt[0], xlt[1], xlt[2], xlt[3]}}) && !ip_all_zero(Ip4w{{xlt[4], xlt[5], xlt[6], xlt[7]}});
    }
    template <typename S> NF_DEV void xlat(S& s) const {                // decode_protobuf.go:158-167
        if (!xlated()) return;
        lit(s, ",\"XlatDstAddr\":\""); ip_text(s, Ip4w{{xlt[4], xlt[5], xlt[6], xlt[7]}}); s.put('"');
        if (xlt[8] >> 16) { lit(s, ",\"XlatDstPort\":"); dec<5>(s, xlt[8] >> 16); }
        lit(s, ",\"XlatSrcAddr\":\""); ip_text(s, Ip4w{{xlt[0], xlt[1], xlt[2], xlt[3]}}); s.put('"');
        if (xlt[8] & 0xffffu) { lit(s, ",\"XlatSrcPort\":"); dec<5>(s, xlt[8] & 0xffffu); }
    }
    template <typename S> NF_DEV void zone(S& s) const {
        if (xlated()) { lit(s, ",\"ZoneId\":"); dec<5>(s, xlt[9] & 0xffffu); }
    }
    template <typename S> NF_DEV void tls_names(S&, const Rec&) const {}     // a record with these keys is deferred; FlpTls has them
    template <typename S> NF_DEV void tls_version(S&, const Rec&) const {}
    template <typename S> NF_DEV void k8s_dst(S&) const {}                   // FlpK8s (nfagg_k8s.h) has the Kubernetes keys
    template <typename S> NF_DEV void k8s_layer(S&) const {}
    template <typename S> NF_DEV void k8s_src(S&) const {}
    static constexpr bool kFlagNames = false;                                // FlpNet (nfagg_net.h) has the transform network rules
    template <typename S> NF_DEV void dst_subnet(S&) const {}
    template <typename S> NF_DEV void flow_direction(S&) const {}
    template <typename S> NF_DEV void src_subnet(S&) const {}
    template <typename S> NF_DEV void conn_meta(S&) const {}                 // FlpConnMeta (nfagg_conn_meta.h) has extract conntrack's keys
};

// FlpContent plus the flow's network events: the table rows nfagg_netev_resolve wrote (PbFeat::ne_rows), each row's JSON
// object rendered once on the host (nfagg_netev.h). The counting pass reads only the lengths.
struct FlpContentNetev : FlpContent {
    static constexpr uint32_t kWindow = kFlpnWindow, kLds = kFlpnLds, kMaxLine = kFlpnMaxLine - kFlpcLineUnreached;
    uint32_t ev[4] = {kNetevNoRow, kNetevNoRow, kNetevNoRow, kNetevNoRow};
    const uint8_t* ne_tab = nullptr;
    const uint8_t* ne_blob = nullptr;
    uint32_t ne_n = 0;

    NF_DEV void load(const PbFeat& F, uint64_t i, uint8_t* name_lds) {
        FlpContent::load(F, i, name_lds);
        netev_rows(F.ne_rows, i, ev);
        ne_tab = F.ne_tab; ne_blob = F.ne_blob; ne_n = F.ne_n;
    }
    template <typename S> NF_DEV void netev(S& s) const {               // decode_protobuf.go:184-186: no event, no key
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (ev[k] < ne_n) {
                if (any) s.put(','); else lit(s, ",\"NetworkEvents\":[");
                any = true;
                const uint4 m = netev_row_blobs(ne_tab, ev[k]);
                put_blob(s, ne_blob + m.x, m.z & 0xffffu);
            }
        if (any) s.put(']');
    }
};

// ---- the launchers. The policy a call selects: its level's layers over the base policy its parts name (flp_policy).
template <typename Feat> struct FlpPolicy { using type = Feat; };
template <typename Base, typename Fn> static hipError_t flp_select_level(FlpLevel level, Fn fn) {
    using Tls = FlpTls<Base>; using K8s = FlpK8s<Tls>; using Net = FlpNet<K8s>;
    switch (level) {
    case FlpLevel::Plain: return fn(FlpPolicy<Base>{});
    case FlpLevel::Tls: return fn(FlpPolicy<Tls>{});
    case FlpLevel::K8s: return fn(FlpPolicy<K8s>{});
    case FlpLevel::Net: return fn(FlpPolicy<Net>{});
    case FlpLevel::Conn: return fn(FlpPolicy<FlpConnMeta<Net>>{});
    }
    return hipErrorInvalidValue;
}
template <typename Fn> static hipError_t flp_select(FlpLevel level, int policy, Fn fn) {
    return policy == 0 ? flp_select_level<FlpPlain>(level, fn) : policy == 1 ? flp_select_level<FlpContent>(level, fn)
         : policy == 2 ? flp_select_level<FlpContentNetev>(level, fn) : hipErrorInvalidValue;
}

hipError_t launch_flp_size(const FlpLineArgs& A, FlpLevel level, uint32_t* d_rows, uint32_t* d_local_off, uint32_t* d_block_sum,
                           uint64_t* d_block_base, uint32_t* d_n_deferred, hipStream_t s) {
    return flp_select(level, flp_policy(A.F), [&](auto policy) {
        return flp_size_as<typename decltype(policy)::type>(A, d_rows, d_local_off, d_block_sum, d_block_base, d_n_deferred, s); });
}

hipError_t launch_flp_write(const FlpLineArgs& A, FlpLevel level, const uint32_t* d_rows, const uint32_t* d_local_off,
                            const uint64_t* d_block_base, void* d_out, uint64_t* d_line_offsets, uint8_t* d_deferred, hipStream_t s) {
    return flp_select(level, flp_policy(A.F), [&](auto policy) {
        return flp_write_as<typename decltype(policy)::type>(A, d_rows, d_local_off, d_block_base, d_out, d_line_offsets, d_deferred, s); });
}

uint32_t flp_max_line(FlpLevel level, int policy) {
    uint32_t longest = 0;
    (void)flp_select(level, policy, [&](auto p) { longest = decltype(p)::type::kMaxLine; return hipSuccess; });
    return longest;
}

// write loki (nfagg_loki_line.h): FlpLoki over the two content policies, in the kernel pair of that header.
hipError_t launch_loki_key_content(const FlpLineArgs& A, const LokiDev& L, const LokiPlanDev& D, hipStream_t s) {
    return A.F.ne_rows ? loki_key_as<LokiOver<FlpContentNetev>>(A, L, D, s) : loki_key_as<LokiOver<FlpContent>>(A, L, D, s);
}
hipError_t launch_loki_write_content(const FlpLineArgs& A, const LokiDev& L, const LokiPlanDev& D, const LokiWriteDev& W, uint32_t m, uint8_t* d_out, hipStream_t s) {
    return A.F.ne_rows ? loki_write_as<LokiOver<FlpContentNetev>>(A, L, D, W, m, d_out, s) : loki_write_as<LokiOver<FlpContent>>(A, L, D, W, m, d_out, s);
}
uint32_t loki_max_entry_content(int policy) {
    return policy == 1 ? LokiOver<FlpContent>::kMaxEntry : policy == 2 ? LokiOver<FlpContentNetev>::kMaxEntry : 0u;
}

}  // namespace nfagg
