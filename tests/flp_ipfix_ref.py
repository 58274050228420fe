"""Independent restatement of flowlogs-pipeline's `write ipfix` stage and of the go-ipfix code it calls, for the tests (no
import of the product). Structurally the Go code: two lists of element objects, one Setter / Default per MapIPFIXKeys entry
applied over the flow's map, one encoder per element type, the exporter's checks and its sequence counter.

  flowlogs-pipeline pkg/pipeline/write/write_ipfix.go     IANAFields, KubeFields, CustomNetworkFields, MapIPFIXKeys,
                                                          prepareTemplate, createDataRecord, sendDataRecord, Write
  flowlogs-pipeline pkg/utils/tcp_flags.go                EncodeTCPFlags / DecodeTCPFlags
  go-ipfix pkg/registry/registry_IANA.go                  ids, types and lengths of the IANA names
  go-ipfix pkg/entities/ie.go:213-330, 624-713            DecodeAndCreateInfoElementWithValue(nil), appendInfoElementValueToBuffer
  go-ipfix pkg/entities/record.go:245-272                 template record: header, field specifiers, enterprise bit and number
  go-ipfix pkg/entities/set.go, pkg/exporter/msg.go       set header, message header
  go-ipfix pkg/exporter/process.go:484-509                the maxMsgSize check, seqNumber counts sent data records

The flow's map is flp_json_content_ref's (RecordToMap and the keys of the feature parts) plus flp_json_k8s_ref.enrich for both
addresses. Also here: a template-driven decoder (parse the template message, decode data messages by it)."""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_content_ref as RC  # noqa: E402
import flp_json_k8s_ref as K  # noqa: E402
from flp_json_ref import record_to_map  # noqa: E402

# entities/ie.go:26-50: IEDataType
U8, U16, U32, U64, F64, MAC, STRING, DT_MS, IPV4, IPV6 = 1, 2, 3, 4, 10, 12, 13, 15, 18, 19
VARIABLE = 65535
# registry_IANA.go: name -> (element id, type, length)
IANA = {
    "octetDeltaCount": (1, U64, 8), "packetDeltaCount": (2, U64, 8), "protocolIdentifier": (4, U8, 1), "tcpControlBits": (6, U16, 2),
    "sourceTransportPort": (7, U16, 2), "sourceIPv4Address": (8, IPV4, 4), "destinationTransportPort": (11, U16, 2),
    "destinationIPv4Address": (12, IPV4, 4), "sourceIPv6Address": (27, IPV6, 16), "destinationIPv6Address": (28, IPV6, 16),
    "sourceMacAddress": (56, MAC, 6), "flowDirection": (61, U8, 1), "destinationMacAddress": (80, MAC, 6),
    "interfaceName": (82, STRING, VARIABLE), "flowStartMilliseconds": (152, DT_MS, 8), "flowEndMilliseconds": (153, DT_MS, 8),
    "icmpTypeIPv4": (176, U8, 1), "icmpCodeIPv4": (177, U8, 1), "icmpTypeIPv6": (178, U8, 1), "icmpCodeIPv6": (179, U8, 1),
    "nextHeaderIPv6": (193, U8, 1), "postNATSourceIPv4Address": (225, IPV4, 4), "postNATDestinationIPv4Address": (226, IPV4, 4),
    "postNAPTSourceTransportPort": (227, U16, 2), "postNAPTDestinationTransportPort": (228, U16, 2), "ethernetType": (256, U16, 2),
    "postNATSourceIPv6Address": (281, IPV6, 16), "postNATDestinationIPv6Address": (282, IPV6, 16), "selectorAlgorithm": (304, U16, 2),
    "samplingProbability": (311, F64, 8),
}
IANA_FIELDS = ["ethernetType", "flowDirection", "sourceMacAddress", "destinationMacAddress", "protocolIdentifier", "sourceTransportPort",
               "destinationTransportPort", "octetDeltaCount", "flowStartMilliseconds", "flowEndMilliseconds", "packetDeltaCount",
               "interfaceName", "tcpControlBits", "postNAPTSourceTransportPort", "postNAPTDestinationTransportPort", "selectorAlgorithm",
               "samplingProbability"]
IPV4_IANA_FIELDS = ["sourceIPv4Address", "destinationIPv4Address", "icmpTypeIPv4", "icmpCodeIPv4", "postNATSourceIPv4Address",
                    "postNATDestinationIPv4Address"] + IANA_FIELDS
IPV6_IANA_FIELDS = ["sourceIPv6Address", "destinationIPv6Address", "nextHeaderIPv6", "icmpTypeIPv6", "icmpCodeIPv6",
                    "postNATSourceIPv6Address", "postNATDestinationIPv6Address"] + IANA_FIELDS
KUBE_FIELDS = [("sourcePodNamespace", 7733, STRING, VARIABLE), ("sourcePodName", 7734, STRING, VARIABLE),
               ("destinationPodNamespace", 7735, STRING, VARIABLE), ("destinationPodName", 7736, STRING, VARIABLE),
               ("sourceNodeName", 7737, STRING, VARIABLE), ("destinationNodeName", 7738, STRING, VARIABLE)]
CUSTOM_NETWORK_FIELDS = [("timeFlowRttNs", 7740, U64, 8), ("interfaces", 7741, STRING, VARIABLE), ("directions", 7742, STRING, VARIABLE)]
IPV6_TYPE = 0x86DD
TCP_FLAGS = [(1, b"FIN"), (2, b"SYN"), (4, b"RST"), (8, b"PSH"), (16, b"ACK"), (32, b"URG"), (64, b"ECE"), (128, b"CWR"), (256, b"SYN_ACK"),
             (512, b"FIN_ACK"), (1024, b"RST_ACK")]
IPV4_ZERO, IPV6_ZERO = bytes(4), bytes(16)


def encode_tcp_flags(flags) -> int:
    m = {name: v for v, name in TCP_FLAGS}
    bf = 0
    for f in flags or []:
        bf |= m.get(f, 0)
    return bf


def decode_tcp_flags(bitfield: int):
    return [name for v, name in TCP_FLAGS if bitfield & v]


class IpError(Exception):
    pass


def parse_ip(text: bytes):
    """net.ParseIP for the texts net.IP.String() writes: a dotted quad gives the 16-byte v4-mapped form, IPv6 text 16 bytes."""
    s = text.decode()
    if ":" not in s:
        q = [int(x) for x in s.split(".")]
        assert len(q) == 4
        return bytes(10) + b"\xff\xff" + bytes(q)
    head, sep, tail = s.partition("::")
    hg = [int(x, 16) for x in head.split(":") if x]
    tg = [int(x, 16) for x in tail.split(":") if x] if sep else []
    g = hg + [0] * (8 - len(hg) - len(tg)) + tg if sep else hg
    assert len(g) == 8
    return b"".join(struct.pack(">H", x) for x in g)


def to4(ip):
    """net.IP.To4()."""
    if ip is None:
        return None
    if len(ip) == 4:
        return bytes(ip)
    if len(ip) == 16 and ip[:10] == bytes(10) and ip[10:12] == b"\xff\xff":
        return bytes(ip[12:])
    return None


def to16(ip):
    if ip is None:
        return None
    if len(ip) == 4:
        return bytes(10) + b"\xff\xff" + bytes(ip)
    return bytes(ip) if len(ip) == 16 else None


def parse_mac(text: bytes) -> bytes:
    return bytes(int(x, 16) for x in text.decode().split(":"))


class Element:
    """entities.InfoElementWithValue as DecodeAndCreateInfoElementWithValue(element, nil) makes it."""

    def __init__(self, name, ie_id, dtype, length, enterprise=0):
        self.name, self.id, self.dtype, self.len, self.enterprise = name, ie_id, dtype, length, enterprise
        self.value = b"" if dtype == STRING else None if dtype in (MAC, IPV4, IPV6) else 0.0 if dtype == F64 else 0

    def append(self, buf: bytearray):
        """appendInfoElementValueToBuffer (ie.go:624-713)."""
        t, v = self.dtype, self.value
        if t == U8:
            buf.append(v & 0xFF)
        elif t == U16:
            buf += struct.pack(">H", v & 0xFFFF)
        elif t == U32:
            buf += struct.pack(">I", v & 0xFFFFFFFF)
        elif t in (U64, DT_MS):
            buf += struct.pack(">Q", v & ((1 << 64) - 1))
        elif t == F64:
            buf += struct.pack(">d", v)
        elif t == MAC:
            buf += v or b""
        elif t == IPV4:
            a = to4(v)
            if a is None:
                raise IpError("provided IP does not belong to IPv4 address family")
            buf += a
        elif t == IPV6:
            a = to16(v)
            if a is None:
                raise IpError("provided IPv6 address is not of correct length")
            buf += a
        elif t == STRING:
            if len(v) < 255:
                buf.append(len(v))
            else:
                assert len(v) <= 0xFFFF
                buf.append(255)
                buf += struct.pack(">H", len(v))
            buf += v
        else:
            raise AssertionError(t)

    def get_length(self) -> int:
        """ie_value.go: the element's length; a string's with its one- or three-byte prefix."""
        if self.dtype == STRING:
            return len(self.value) + (1 if len(self.value) < 255 else 3)
        return self.len


def _set(e, v):
    e.value = v


def _set_first_dir(e, rec):
    if isinstance(rec, list) and len(rec) > 0:
        e.value = rec[0] & 0xFF


def _set_directions(e, rec):
    if isinstance(rec, list) and len(rec) > 0:
        e.value = b",".join(str(int(d)).encode() for d in rec)


def _set_first_intf(e, rec):
    if isinstance(rec, list) and len(rec) > 0:
        e.value = bytes(rec[0])


def _set_interfaces(e, rec):
    if isinstance(rec, list):
        e.value = b",".join(bytes(x) for x in rec)


def _set_flags(e, rec):
    if isinstance(rec, list):                          # []string: decoded, re-encode for ipfix
        e.value = encode_tcp_flags(rec) & 0xFFFF
    elif isinstance(rec, int):
        e.value = rec


def _set_selector(e, rec):
    if isinstance(rec, int) and rec > 0:
        e.value = 4


def _set_probability(e, rec):
    if isinstance(rec, int) and rec > 0:
        e.value = 1.0 / float(rec)


_ip = lambda e, rec: _set(e, parse_ip(rec))            # noqa: E731  elt.SetIPAddressValue(net.ParseIP(rec.(string)))
_mac = lambda e, rec: _set(e, parse_mac(rec))          # noqa: E731
_u64 = lambda e, rec: _set(e, rec & ((1 << 64) - 1))   # noqa: E731  uint64(rec.(int64))
# MapIPFIXKeys: element name -> (map key, Setter, Default or None)
MAP_IPFIX_KEYS = {
    "sourceIPv4Address": (b"SrcAddr", _ip, None), "destinationIPv4Address": (b"DstAddr", _ip, None),
    "sourceIPv6Address": (b"SrcAddr", _ip, None), "destinationIPv6Address": (b"DstAddr", _ip, None),
    "nextHeaderIPv6": (b"Proto", _set, None), "sourceMacAddress": (b"SrcMac", _mac, None), "destinationMacAddress": (b"DstMac", _mac, None),
    "ethernetType": (b"Etype", _set, None), "flowDirection": (b"IfDirections", _set_first_dir, None),
    "directions": (b"IfDirections", _set_directions, None), "protocolIdentifier": (b"Proto", _set, None),
    "sourceTransportPort": (b"SrcPort", _set, None), "destinationTransportPort": (b"DstPort", _set, None),
    "octetDeltaCount": (b"Bytes", _set, None), "flowStartMilliseconds": (b"TimeFlowStartMs", _u64, None),
    "flowEndMilliseconds": (b"TimeFlowEndMs", _u64, None), "packetDeltaCount": (b"Packets", _set, None),
    "interfaceName": (b"Interfaces", _set_first_intf, None), "tcpControlBits": (b"Flags", _set_flags, None),
    "icmpTypeIPv4": (b"IcmpType", _set, None), "icmpCodeIPv4": (b"IcmpCode", _set, None),
    "icmpTypeIPv6": (b"IcmpType", _set, None), "icmpCodeIPv6": (b"IcmpCode", _set, None),
    "interfaces": (b"Interfaces", _set_interfaces, None),
    "sourcePodNamespace": (b"SrcK8S_Namespace", _set, None), "sourcePodName": (b"SrcK8S_Name", _set, None),
    "destinationPodNamespace": (b"DstK8S_Namespace", _set, None), "destinationPodName": (b"DstK8S_Name", _set, None),
    "sourceNodeName": (b"SrcK8S_HostName", _set, None), "destinationNodeName": (b"DstK8S_HostName", _set, None),
    "timeFlowRttNs": (b"TimeFlowRttNs", _u64, None),
    "postNAPTSourceTransportPort": (b"XlatSrcPort", _set, None), "postNAPTDestinationTransportPort": (b"XlatDstPort", _set, None),
    "postNATSourceIPv4Address": (b"XlatSrcAddr", _ip, lambda e: _set(e, IPV4_ZERO)),
    "postNATDestinationIPv4Address": (b"XlatDstAddr", _ip, lambda e: _set(e, IPV4_ZERO)),
    "postNATSourceIPv6Address": (b"XlatSrcAddr", _ip, lambda e: _set(e, IPV6_ZERO)),
    "postNATDestinationIPv6Address": (b"XlatDstAddr", _ip, lambda e: _set(e, IPV6_ZERO)),
    "selectorAlgorithm": (b"Sampling", _set_selector, None), "samplingProbability": (b"Sampling", _set_probability, None),
}


def prepare_template(template_id: int, enterprise_id: int, v6: bool):
    """prepareTemplate: the template record's bytes (record header and field specifiers) and the element list."""
    elements = [Element(name, *IANA[name]) for name in (IPV6_IANA_FIELDS if v6 else IPV4_IANA_FIELDS)]
    if enterprise_id != 0:
        elements += [Element(name, i, t, ln, enterprise_id) for name, i, t, ln in KUBE_FIELDS + CUSTOM_NETWORK_FIELDS]
    rec = bytearray(struct.pack(">HH", template_id, len(elements)))
    for e in elements:
        if e.enterprise:
            rec += struct.pack(">HHI", e.id | 0x8000, e.len, e.enterprise)
        else:
            rec += struct.pack(">HH", e.id, e.len)
    return bytes(rec), elements


def message(set_id: int, records: bytes, obs_domain: int, seq: int, export_time: int) -> bytes:
    """WriteIPFIXMsgToBuffer: message header, set header, the records."""
    set_len = 4 + len(records)
    return struct.pack(">HHIII", 10, 16 + set_len, export_time & 0xFFFFFFFF, seq & 0xFFFFFFFF, obs_domain) + struct.pack(">HH", set_id, set_len) + records


class WriteIpfix:
    """NewWriteIpfix and Write. send(message) takes every message that goes out; failures are (flow index, status) with status 1
    for an address family error and 2 for a message over max_msg_size."""

    def __init__(self, send, enterprise_id=0, max_msg_size=65535, obs_domain=1, export_time=0):
        self.send, self.enterprise_id, self.max_msg_size, self.obs_domain = send, enterprise_id, max_msg_size, obs_domain
        self.seq = 0
        self.template_id = 255                                       # startTemplateID
        self.id_v4 = self.new_template_id()
        self.tpl_v4, self.entities_v4 = prepare_template(self.id_v4, enterprise_id, False)
        self.id_v6 = self.new_template_id()
        self.tpl_v6, self.entities_v6 = prepare_template(self.id_v6, enterprise_id, True)
        self.send_templates(export_time)
        self.failures = []
        self.count = 0

    def new_template_id(self):
        self.template_id += 1
        return self.template_id

    def send_templates(self, export_time):
        for tpl in (self.tpl_v4, self.tpl_v6):
            self.send(message(2, tpl, self.obs_domain, self.seq, export_time))

    @staticmethod
    def create_data_record(flow: dict, elements):
        for e in elements:
            mapping = MAP_IPFIX_KEYS.get(e.name)
            if mapping is None:
                continue
            key, setter, default = mapping
            value = flow.get(key)                      # a missing key reads as nil; DecodeTCPFlags' empty slice is not nil
            if value is not None:
                setter(e, value)
            elif default is not None:
                default(e)

    def write(self, flow: dict, export_time: int, encode: bool = True):
        """Write -> sendDataRecord. Returns the message, or None with the failure recorded. encode=False (for long streams of
        which a test compares a sample): the same setters, checks and counting, but the bytes are not built and b"?" stands
        for a sent message."""
        v6 = flow[b"Etype"] == IPV6_TYPE
        template_id, elements = (self.id_v6, self.entities_v6) if v6 else (self.id_v4, self.entities_v4)
        self.create_data_record(flow, elements)
        index = self.count
        self.count += 1
        set_len = 4 + sum(e.get_length() for e in elements)
        assert 16 + set_len <= 65535
        if not encode:
            if any((e.dtype == IPV4 and to4(e.value) is None) or (e.dtype == IPV6 and to16(e.value) is None) for e in elements):
                self.failures.append((index, 1))
                return None
            if 16 + set_len > self.max_msg_size:
                self.failures.append((index, 2))
                return None
            self.seq = (self.seq + 1) & 0xFFFFFFFF
            return b"?"
        body = bytearray()
        try:
            for e in elements:
                e.append(body)
        except IpError:
            self.failures.append((index, 1))
            return None
        msg = message(template_id, bytes(body), self.obs_domain, self.seq, export_time)
        assert len(msg) == 16 + set_len
        if len(msg) > self.max_msg_size:
            self.failures.append((index, 2))
            return None
        self.send(msg)
        self.seq = (self.seq + 1) & 0xFFFFFFFF
        return msg

    def elements(self, v6: bool) -> dict:
        return {e.name: e.value for e in (self.entities_v6 if v6 else self.entities_v4)}


def flow_map(rec: bytes, parts: dict, k8s_table: dict, now, mono, names, unknown=b"unknown", flags_decoded=False, memo=None):
    """The GenericMap the writer sees for one flow: RecordToMap with the feature parts' keys, the Kubernetes enrichment of both
    addresses, and with flags_decoded the decode_tcp_flags rule applied to Flags."""
    out = record_to_map(rec, now, mono, names, None, 0, unknown, memo)
    RC.add_content(out, parts)
    if k8s_table is not None:
        K.enrich(out, b"SrcAddr", b"SrcK8S", k8s_table)
        K.enrich(out, b"DstAddr", b"DstK8S", k8s_table)
    if flags_decoded and b"Flags" in out:
        out[b"Flags"] = decode_tcp_flags(out[b"Flags"])
    return out


def run(writer: WriteIpfix, records, now, mono, names, export_time, present=None, parts=None, k8s_entries=None, unknown=b"unknown",
        flags_decoded=False, only=None):
    """One call's flows through `writer`. Returns (messages: list of bytes, b"" for a failed flow; status: list). only: the
    indexes whose bytes are built (the others' messages are b"?"); equal flows share their map."""
    import numpy as np
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1, 144)
    table = K.table_of(k8s_entries) if k8s_entries is not None else None
    memo, maps = {}, {}
    first = writer.count
    msgs = []
    for i in range(len(raw)):
        rec, fp = raw[i].tobytes(), RC.flow_parts(present, parts, i)
        key = (rec, tuple(sorted(fp.items())))
        if key not in maps:
            maps[key] = flow_map(rec, fp, table, now, mono, names, unknown, flags_decoded, memo)
        msg = writer.write(maps[key], export_time, only is None or i in only)
        msgs.append(msg or b"")
    failed = {i - first: st for i, st in writer.failures if i >= first}
    return msgs, [failed.get(i, 0) for i in range(len(raw))]


# ---- the template-driven decoder
def parse_template(msg: bytes):
    """A template message -> (template id, [(element id, length, enterprise number)])."""
    version, length, _, _, _ = struct.unpack_from(">HHIII", msg, 0)
    set_id, set_len = struct.unpack_from(">HH", msg, 16)
    assert version == 10 and length == len(msg) and set_id == 2 and set_len == len(msg) - 16
    tid, count = struct.unpack_from(">HH", msg, 20)
    p, fields = 24, []
    for _ in range(count):
        eid, ln = struct.unpack_from(">HH", msg, p)
        p += 4
        ent = 0
        if eid & 0x8000:
            ent, = struct.unpack_from(">I", msg, p)
            p += 4
        fields.append((eid & 0x7FFF, ln, ent))
    assert p == len(msg)
    return tid, fields


def decode_data(msg: bytes, templates: dict):
    """A data message with one record -> (header dict, [(element id, enterprise, raw value bytes)]); templates: {id: fields}."""
    version, length, export_time, seq, domain = struct.unpack_from(">HHIII", msg, 0)
    set_id, set_len = struct.unpack_from(">HH", msg, 16)
    assert version == 10 and length == len(msg) and set_len == len(msg) - 16
    p, out = 20, []
    for eid, ln, ent in templates[set_id]:
        if ln == VARIABLE:
            ln = msg[p]
            p += 1
            if ln == 255:
                ln, = struct.unpack_from(">H", msg, p)
                p += 2
        out.append((eid, ent, msg[p:p + ln]))
        p += ln
    assert p == len(msg), "the record does not end with the message"
    return dict(export_time=export_time, seq=seq, domain=domain, template=set_id), out
