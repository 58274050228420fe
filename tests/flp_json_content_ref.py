"""Independent restatement of the direct-FLP stdout line of a MapTracer flow (a full model.BpfFlowContent), for the tests:
the map of tests/flp_json_ref.py plus the keys the feature parts add (no import of the product):

  pkg/model/record.go:116-125                NewRecord: DNSLatency, TimeFlowRtt
  pkg/decode/decode_protobuf.go:130-192      RecordToMap, the feature parts
  pkg/decode/decode_protobuf.go:199-464      TCPStateToStr, PktDropCauseToStr, DNSRcodeToStr
  pkg/utils/networkevents/network_events.go  causes, DropReasonCodeToString
  pkg/utils/utils.go:18-60                   DNSRawNameToDotted
  pkg/model/record.go:233-238, 259-270       AllZeroIP, QuicVersionToString

A flow's parts are a dict {"additional" | "dns" | "drops" | "xlat" | "quic": the part's bytes (bpf/types.h layout)}; a kind
that is missing is a nil pointer of BpfFlowContent. Network events take a decoder the encoder does not have: with a nil
decoder NewRecord leaves NetworkMonitorEventsMD empty (record.go:126), so they add nothing. The name tables are restated
once, here."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flp_json_ref import go_ip, is_deferred, jsoniter_string, marshal_sorted, record_to_map  # noqa: E402,F401

FEAT = {"additional": 1, "dns": 2, "drops": 4, "network_events": 8, "xlat": 16, "quic": 32}      # NFAGG_FEAT_*
SIZES = {"additional": 32, "dns": 64, "drops": 32, "xlat": 56, "quic": 24}
_ADDITIONAL = struct.Struct("<QQQiHBx")
_DNS = struct.Struct("<QQQHHHB32sx")
_DROPS = struct.Struct("<QQHHIHHB3x")
_XLAT = struct.Struct("<QQ16s16sHHHH")
_QUIC = struct.Struct("<QQIHBB")
assert [s.size for s in (_ADDITIONAL, _DNS, _DROPS, _XLAT, _QUIC)] == [32, 64, 32, 56, 24]

RCODES = ["NoError", "FormErr", "ServFail", "NXDomain", "NotImp", "Refused", "YXDomain", "YXRRSet", "NXRRSet", "NotAuth", "NotZone"]
TCP_STATES = ["TCP_ESTABLISHED", "TCP_SYN_SENT", "TCP_SYN_RECV", "TCP_FIN_WAIT1", "TCP_FIN_WAIT2", "TCP_CLOSE", "TCP_CLOSE_WAIT",
              "TCP_LAST_ACK", "TCP_LISTEN", "TCP_CLOSING", "TCP_NEW_SYN_RECV"]                        # states 1..11
CORE_CAUSES = """NOT_SPECIFIED NO_SOCKET PKT_TOO_SMALL TCP_CSUM SOCKET_FILTER UDP_CSUM NETFILTER_DROP OTHERHOST IP_CSUM IP_INHDR
IP_RPFILTER UNICAST_IN_L2_MULTICAST XFRM_POLICY IP_NOPROTO SOCKET_RCVBUFF PROTO_MEM TCP_MD5NOTFOUND TCP_MD5UNEXPECTED
TCP_MD5FAILURE SOCKET_BACKLOG TCP_FLAGS TCP_ZEROWINDOW TCP_OLD_DATA TCP_OVERWINDOW TCP_OFOMERGE TCP_RFC7323_PAWS
TCP_INVALID_SEQUENCE TCP_RESET TCP_INVALID_SYN TCP_CLOSE TCP_FASTOPEN TCP_OLD_ACK TCP_TOO_OLD_ACK TCP_ACK_UNSENT_DATA
TCP_OFO_QUEUE_PRUNE TCP_OFO_DROP IP_OUTNOROUTES BPF_CGROUP_EGRESS IPV6DISABLED NEIGH_CREATEFAIL NEIGH_FAILED NEIGH_QUEUEFULL
NEIGH_DEAD TC_EGRESS QDISC_DROP CPU_BACKLOG XDP TC_INGRESS UNHANDLED_PROTO SKB_CSUM SKB_GSO_SEG SKB_UCOPY_FAULT DEV_HDR
DEV_READY FULL_RING NOMEM HDR_TRUNC TAP_FILTER TAP_TXFILTER ICMP_CSUM INVALID_PROTO IP_INADDRERRORS IP_INNOROUTES PKT_TOO_BIG
DUP_FRAG FRAG_REASM_TIMEOUT FRAG_TOO_FAR TCP_MINTTL IPV6_BAD_EXTHDR IPV6_NDISC_FRAG IPV6_NDISC_HOP_LIMIT IPV6_NDISC_BAD_CODE
IPV6_NDISC_BAD_OPTIONS IPV6_NDISC_NS_OTHERHOST QUEUE_PURGE TC_COOKIE_ERROR PACKET_SOCK_ERROR TC_CHAIN_NOTFOUND
TC_RECLASSIFY_LOOP""".split()                                                                         # core subsystem 2..80
OVS_CAUSES = ["LAST_ACTION", "ACTION_ERROR", "EXPLICIT", "EXPLICIT_WITH_ERROR", "METER", "RECURSION_LIMIT", "DEFERRED_LIMIT",
              "FRAG_L2_TOO_LONG", "FRAG_INVALID_PROTO", "CONNTRACK", "IP_TTL"]                         # (3 << 16) + 1..11
NETWORK_EVENT_CAUSES = ["Unknown", "EgressFirewall", "AdminNetworkPolicy", "BaselineAdminNetworkPolicy", "NetworkPolicy",
                        "MulticastNS", "MulticastCluster", "NetpolNode", "NetpolNamespace", "UDNIsolation"]   # (1 << 24) + 0..9
assert len(CORE_CAUSES) == 79 and len(OVS_CAUSES) == 11


def dns_rcode(rcode: int) -> bytes:
    return (RCODES[rcode] if rcode <= 10 else "UnDefined").encode()        # cases 16..21 cannot match a 4-bit value


def tcp_state(state: int) -> bytes:
    return (TCP_STATES[state - 1] if 1 <= state <= 11 else "TCP_INVALID_STATE").encode()


def drop_cause(cause: int) -> bytes:
    if 2 <= cause <= 80:
        return b"SKB_DROP_REASON_" + CORE_CAUSES[cause - 2].encode()
    if (3 << 16) + 1 <= cause <= (3 << 16) + 11:
        return b"OVS_DROP_" + OVS_CAUSES[cause - (3 << 16) - 1].encode()
    if (1 << 24) <= cause < (1 << 24) + len(NETWORK_EVENT_CAUSES):
        return b"NetworkEvent_" + NETWORK_EVENT_CAUSES[cause - (1 << 24)].encode()
    return b"SKB_DROP_UNKNOWN_CAUSE"


def dns_dotted(raw: bytes) -> bytes:
    b = raw.split(b"\0", 1)[0]
    out, i = [], 0
    while i < len(b):
        n = b[i]
        if n == 0 or n & 0xC0 == 0xC0:
            break
        i += 1
        if i + n > len(b):
            break
        out.append(b[i:i + n])
        i += n
    return b".".join(out)


def all_zero_ip(ip: bytes) -> bool:                  # ip.Equal(net.IPv4zero) || ip.Equal(net.IPv6zero), ip of 16 bytes
    return ip == bytes(16) or ip == bytes(10) + b"\xff\xff" + bytes(4)


def _i64(v):
    return v - (1 << 64) if v >> 63 else v


def _go_div(a, b):                                   # Go's integer division truncates towards zero
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def add_content(out: dict, parts: dict) -> dict:
    """The keys decode_protobuf.go:130-192 adds to RecordToMap's map `out`, for the parts that are present."""
    if "dns" in parts:
        _, _, latency, dns_id, flags, _, errno, name = _DNS.unpack(parts["dns"])
        if errno:
            out[b"DnsErrno"] = errno
        if dns_id:
            out[b"DnsId"], out[b"DnsFlags"], out[b"DnsFlagsResponseCode"] = dns_id, flags, dns_rcode(flags & 0xF)
            out[b"DnsLatencyMs"] = _go_div(_i64(latency), 10**6)            # time.Duration(latency).Milliseconds()
            dotted = dns_dotted(name)
            if dotted:
                out[b"DnsName"] = dotted
    if "drops" in parts:
        _, _, nbytes, packets, cause, flags, _, state = _DROPS.unpack(parts["drops"])
        if cause:
            out[b"PktDropBytes"], out[b"PktDropPackets"], out[b"PktDropLatestFlags"] = nbytes, packets, flags
            out[b"PktDropLatestState"], out[b"PktDropLatestDropCause"] = tcp_state(state), drop_cause(cause)
    if "xlat" in parts:
        _, _, saddr, daddr, sport, dport, zone, _ = _XLAT.unpack(parts["xlat"])
        if not all_zero_ip(daddr) and not all_zero_ip(saddr):
            out[b"ZoneId"] = zone
            if sport:
                out[b"XlatSrcPort"] = sport
            if dport:
                out[b"XlatDstPort"] = dport
            out[b"XlatSrcAddr"], out[b"XlatDstAddr"] = go_ip(saddr), go_ip(daddr)
    if "additional" in parts:
        _, _, rtt, ret, _, encrypted = _ADDITIONAL.unpack(parts["additional"])
        if ret:
            out[b"IPSecRetCode"], out[b"IPSecStatus"] = ret, b"error"
        elif encrypted:
            out[b"IPSecRetCode"], out[b"IPSecStatus"] = 0, b"success"
        if rtt:
            out[b"TimeFlowRttNs"] = _i64(rtt)
    if "quic" in parts:
        _, _, version, _, long_hdr, short_hdr = _QUIC.unpack(parts["quic"])
        out[b"QuicVersion"] = {0: b"QUIC v1", 1: b"QUIC v2"}.get(version, b"QUIC Unknown (%d)" % version)
        out[b"QuicSeenLongHdr"], out[b"QuicSeenShortHdr"] = long_hdr, short_hdr
    return out


def flow_parts(present, parts, i):
    """The parts of flow i out of struct-of-arrays inputs: present (FEAT bits per flow, or None) and parts {kind: array of n
    structs, or None}; a kind without an array is absent whatever present says."""
    if present is None:
        return {}
    out = {}
    for kind, size in SIZES.items():
        a = (parts or {}).get(kind)
        if a is not None and int(present[i]) & FEAT[kind]:
            out[kind] = np.ascontiguousarray(a).view(np.uint8).reshape(-1, size)[i].tobytes()
    return out


def encode(records, present, parts, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown=b"unknown"):
    """The lines of these flows. Returns (bytes, offsets uint64[n + 1], deferred uint8[n]) as flp_json_ref.encode does."""
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1, 144)
    n = len(raw)
    blob = raw.tobytes()
    off = np.zeros(n + 1, dtype=np.uint64)
    deferred = np.zeros(n, dtype=np.uint8)
    memo, lines, pos = {}, [], 0
    for i in range(n):
        rec = blob[144 * i:144 * i + 144]
        if is_deferred(rec):
            deferred[i] = 1
        else:
            m = record_to_map(rec, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown, memo)
            line = marshal_sorted(add_content(m, flow_parts(present, parts, i))) + b"\n"
            lines.append(line)
            pos += len(line)
        off[i + 1] = pos
    return b"".join(lines), off, deferred
