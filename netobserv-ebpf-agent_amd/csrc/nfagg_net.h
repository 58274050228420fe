// nfagg_net.h — three more rules of flowlogs-pipeline's transform network stage on the direct-FLP JSON line, as a feature
// policy on top of FlpK8s<FlpTls<Base>> that k_flp_size / k_flp_write (nfagg_flp_line.h) run: reinterpret_direction
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
    NF_DEV void load_joins(const FlpJoins& J, uint64_t i) { Base::load_joins(J, i); load_net(J.N, J.net_rows, i); }
    template <typename S> NF_DEV void src_subnet(S& s) const { if (net_len[0]) put_blob(s, net_blob + (size_t)net_off[0] * 16, net_len[0]); }
    template <typename S> NF_DEV void dst_subnet(S& s) const { if (net_len[1]) put_blob(s, net_blob + (size_t)net_off[1] * 16, net_len[1]); }
    template <typename S> NF_DEV void flow_direction(S& s) const {
        if (dir <= 2) { lit(s, ",\"FlowDirection\":"); s.put((uint8_t)('0' + dir)); }
    }
    template <typename S> NF_DEV void flags_value(S& s, uint32_t v) const {
        if (names) tcp_flag_names(s, v); else dec<5>(s, v);
    }
};

}  // namespace nfagg
