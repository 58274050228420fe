// nfagg_flp_names.h — the name tables of the direct-FLP encoders: the text RecordToMap prints for a DNS response code, a TCP
// state and a drop cause. One copy for both sides: nfagg_flp_content.hip packs it into its constant blob, nfagg_flp_enum_name
// (the host's view, for the label values of the flow metrics) reads the strings as they are. Host + device.
#pragma once
#include <stdint.h>
#include "nfagg_hash.h"

namespace nfagg {

// ---- the name tables: DNSRcodeToStr, TCPStateToStr, PktDropCauseToStr (decode_protobuf.go:199-464) and the causes of
// networkevents.DropReasonCodeToString (network_events.go:17-28,133-138) behind their "NetworkEvent_" prefix
constexpr const char* const kFlpNames[] = {
    // DNSRcodeToStr of a 4-bit value: 0..10, everything else "UnDefined" (its cases 16..21 cannot match)
    "NoError", "FormErr", "ServFail", "NXDomain", "NotImp", "Refused", "YXDomain", "YXRRSet", "NXRRSet", "NotAuth", "NotZone",
    "UnDefined",
    // TCPStateToStr: the fallback, then states 1..11
    "TCP_INVALID_STATE", "TCP_ESTABLISHED", "TCP_SYN_SENT", "TCP_SYN_RECV", "TCP_FIN_WAIT1", "TCP_FIN_WAIT2", "TCP_CLOSE",
    "TCP_CLOSE_WAIT", "TCP_LAST_ACK", "TCP_LISTEN", "TCP_CLOSING", "TCP_NEW_SYN_RECV",
    // PktDropCauseToStr: the core subsystem's causes 2..80
    "SKB_DROP_REASON_NOT_SPECIFIED", "SKB_DROP_REASON_NO_SOCKET", "SKB_DROP_REASON_PKT_TOO_SMALL", "SKB_DROP_REASON_TCP_CSUM",
    "SKB_DROP_REASON_SOCKET_FILTER", "SKB_DROP_REASON_UDP_CSUM", "SKB_DROP_REASON_NETFILTER_DROP", "SKB_DROP_REASON_OTHERHOST",
    "SKB_DROP_REASON_IP_CSUM", "SKB_DROP_REASON_IP_INHDR", "SKB_DROP_REASON_IP_RPFILTER",
    "SKB_DROP_REASON_UNICAST_IN_L2_MULTICAST", "SKB_DROP_REASON_XFRM_POLICY", "SKB_DROP_REASON_IP_NOPROTO",
    "SKB_DROP_REASON_SOCKET_RCVBUFF", "SKB_DROP_REASON_PROTO_MEM", "SKB_DROP_REASON_TCP_MD5NOTFOUND",
    "SKB_DROP_REASON_TCP_MD5UNEXPECTED", "SKB_DROP_REASON_TCP_MD5FAILURE", "SKB_DROP_REASON_SOCKET_BACKLOG",
    "SKB_DROP_REASON_TCP_FLAGS", "SKB_DROP_REASON_TCP_ZEROWINDOW", "SKB_DROP_REASON_TCP_OLD_DATA",
    "SKB_DROP_REASON_TCP_OVERWINDOW", "SKB_DROP_REASON_TCP_OFOMERGE", "SKB_DROP_REASON_TCP_RFC7323_PAWS",
    "SKB_DROP_REASON_TCP_INVALID_SEQUENCE", "SKB_DROP_REASON_TCP_RESET", "SKB_DROP_REASON_TCP_INVALID_SYN",
    "SKB_DROP_REASON_TCP_CLOSE", "SKB_DROP_REASON_TCP_FASTOPEN", "SKB_DROP_REASON_TCP_OLD_ACK",
    "SKB_DROP_REASON_TCP_TOO_OLD_ACK", "SKB_DROP_REASON_TCP_ACK_UNSENT_DATA", "SKB_DROP_REASON_TCP_OFO_QUEUE_PRUNE",
    "SKB_DROP_REASON_TCP_OFO_DROP", "SKB_DROP_REASON_IP_OUTNOROUTES", "SKB_DROP_REASON_BPF_CGROUP_EGRESS",
    "SKB_DROP_REASON_IPV6DISABLED", "SKB_DROP_REASON_NEIGH_CREATEFAIL", "SKB_DROP_REASON_NEIGH_FAILED",
    "SKB_DROP_REASON_NEIGH_QUEUEFULL", "SKB_DROP_REASON_NEIGH_DEAD", "SKB_DROP_REASON_TC_EGRESS", "SKB_DROP_REASON_QDISC_DROP",
    "SKB_DROP_REASON_CPU_BACKLOG", "SKB_DROP_REASON_XDP", "SKB_DROP_REASON_TC_INGRESS", "SKB_DROP_REASON_UNHANDLED_PROTO",
    "SKB_DROP_REASON_SKB_CSUM", "SKB_DROP_REASON_SKB_GSO_SEG", "SKB_DROP_REASON_SKB_UCOPY_FAULT", "SKB_DROP_REASON_DEV_HDR",
    "SKB_DROP_REASON_DEV_READY", "SKB_DROP_REASON_FULL_RING", "SKB_DROP_REASON_NOMEM", "SKB_DROP_REASON_HDR_TRUNC",
    "SKB_DROP_REASON_TAP_FILTER", "SKB_DROP_REASON_TAP_TXFILTER", "SKB_DROP_REASON_ICMP_CSUM", "SKB_DROP_REASON_INVALID_PROTO",
    "SKB_DROP_REASON_IP_INADDRERRORS", "SKB_DROP_REASON_IP_INNOROUTES", "SKB_DROP_REASON_PKT_TOO_BIG", "SKB_DROP_REASON_DUP_FRAG",
    "SKB_DROP_REASON_FRAG_REASM_TIMEOUT", "SKB_DROP_REASON_FRAG_TOO_FAR", "SKB_DROP_REASON_TCP_MINTTL",
    "SKB_DROP_REASON_IPV6_BAD_EXTHDR", "SKB_DROP_REASON_IPV6_NDISC_FRAG", "SKB_DROP_REASON_IPV6_NDISC_HOP_LIMIT",
    "SKB_DROP_REASON_IPV6_NDISC_BAD_CODE", "SKB_DROP_REASON_IPV6_NDISC_BAD_OPTIONS", "SKB_DROP_REASON_IPV6_NDISC_NS_OTHERHOST",
    "SKB_DROP_REASON_QUEUE_PURGE", "SKB_DROP_REASON_TC_COOKIE_ERROR", "SKB_DROP_REASON_PACKET_SOCK_ERROR",
    "SKB_DROP_REASON_TC_CHAIN_NOTFOUND", "SKB_DROP_REASON_TC_RECLASSIFY_LOOP",
    // the Open vSwitch subsystem's causes (3 << 16) + 1..11
    "OVS_DROP_LAST_ACTION", "OVS_DROP_ACTION_ERROR", "OVS_DROP_EXPLICIT", "OVS_DROP_EXPLICIT_WITH_ERROR", "OVS_DROP_METER",
    "OVS_DROP_RECURSION_LIMIT", "OVS_DROP_DEFERRED_LIMIT", "OVS_DROP_FRAG_L2_TOO_LONG", "OVS_DROP_FRAG_INVALID_PROTO",
    "OVS_DROP_CONNTRACK", "OVS_DROP_IP_TTL",
    // network-event causes (1 << 24) + 0..9
    "NetworkEvent_Unknown", "NetworkEvent_EgressFirewall", "NetworkEvent_AdminNetworkPolicy",
    "NetworkEvent_BaselineAdminNetworkPolicy", "NetworkEvent_NetworkPolicy", "NetworkEvent_MulticastNS",
    "NetworkEvent_MulticastCluster", "NetworkEvent_NetpolNode", "NetworkEvent_NetpolNamespace", "NetworkEvent_UDNIsolation",
    "SKB_DROP_UNKNOWN_CAUSE"};
constexpr uint32_t kFlpNameCount = sizeof(kFlpNames) / sizeof(kFlpNames[0]);
constexpr uint32_t kNameRcode = 0, kNameRcodeUndefined = 11, kNameTcpInvalid = 12;
constexpr uint32_t kNameCore = 24, kCoreFirst = 2, kCoreLast = 80;
constexpr uint32_t kNameOvs = kNameCore + (kCoreLast - kCoreFirst + 1), kOvsBase = (3u << 16) + 1, kOvsCount = 11;
constexpr uint32_t kNameNetEvent = kNameOvs + kOvsCount, kNetEventBase = 1u << 24, kNetEventCount = 10;
constexpr uint32_t kNameUnknownCause = kNameNetEvent + kNetEventCount;
static_assert(kNameUnknownCause + 1 == kFlpNameCount, "name table layout");

// The table index of a raw value, as the encoder picks it.
NF_HD uint32_t rcode_name(uint32_t rcode) { return rcode <= 10 ? kNameRcode + rcode : kNameRcodeUndefined; }
NF_HD uint32_t tcp_state_name(uint32_t state) { return kNameTcpInvalid + (state <= 11 ? state : 0u); }
NF_HD uint32_t drop_cause_name(uint32_t cause) {
    if (cause - kCoreFirst <= kCoreLast - kCoreFirst) return kNameCore + (cause - kCoreFirst);
    if (cause - kOvsBase < kOvsCount) return kNameOvs + (cause - kOvsBase);
    if (cause - kNetEventBase < kNetEventCount) return kNameNetEvent + (cause - kNetEventBase);
    return kNameUnknownCause;
}

}  // namespace nfagg
