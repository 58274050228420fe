"""Independent restatement of the reference's IPFIX export, for the tests (no import of the product's encoder):

(a) encoder: pkg/exporter/ipfix.go (StartIPFIXExporter's two templates, setEntities / sendDataRecord / ExportFlows)
    over model.NewRecord (pkg/model/record.go:82-106) and go-ipfix's message writer (exporter/msg.go, entities/ie.go
    encoders, registry_IANA.go IDs and lengths), vectorised with numpy: a million flows take seconds.
(b) decoder: go-ipfix's collecting process (collector/process.go:232-481): message header, one set, template sets
    recorded per observation domain, data records walked field by field in template order, the variable-length rule
    (a length byte < 255, else 255 and a 16-bit length: :455, :500-515).
"""
import struct

import numpy as np

TEMPLATE_ID_V4, TEMPLATE_ID_V6 = 256, 257          # NewTemplateID() from 255 (process.go:477-480): v4 is created first
VARLEN = 65535

# registry_IANA.go: element id -> (name, type, length)
REGISTRY = {
    1: ("octetDeltaCount", "u", 8), 2: ("packetDeltaCount", "u", 8), 4: ("protocolIdentifier", "u", 1),
    6: ("tcpControlBits", "u", 2), 7: ("sourceTransportPort", "u", 2), 8: ("sourceIPv4Address", "ip", 4),
    11: ("destinationTransportPort", "u", 2), 12: ("destinationIPv4Address", "ip", 4), 27: ("sourceIPv6Address", "ip", 16),
    28: ("destinationIPv6Address", "ip", 16), 56: ("sourceMacAddress", "mac", 6), 61: ("flowDirection", "u", 1),
    80: ("destinationMacAddress", "mac", 6), 82: ("interfaceName", "string", VARLEN), 150: ("flowStartSeconds", "u", 4),
    151: ("flowEndSeconds", "u", 4), 152: ("flowStartMilliseconds", "u", 8), 153: ("flowEndMilliseconds", "u", 8),
    176: ("icmpTypeIPv4", "u", 1), 177: ("icmpCodeIPv4", "u", 1), 178: ("icmpTypeIPv6", "u", 1), 179: ("icmpCodeIPv6", "u", 1),
    193: ("nextHeaderIPv6", "u", 1), 256: ("ethernetType", "u", 2),
}
_BY_NAME = {v[0]: k for k, v in REGISTRY.items()}

_COMMON_TAIL = ["octetDeltaCount", "tcpControlBits", "flowStartSeconds", "flowStartMilliseconds", "flowEndSeconds",
                "flowEndMilliseconds", "packetDeltaCount", "interfaceName"]          # AddRecordValuesToTemplate
FIELDS_V4 = ["ethernetType", "flowDirection", "sourceMacAddress", "destinationMacAddress", "sourceIPv4Address",
             "destinationIPv4Address", "protocolIdentifier", "sourceTransportPort", "destinationTransportPort",
             "icmpTypeIPv4", "icmpCodeIPv4"] + _COMMON_TAIL                             # ipfix.go:89-135
FIELDS_V6 = ["ethernetType", "flowDirection", "sourceMacAddress", "destinationMacAddress", "sourceIPv6Address",
             "destinationIPv6Address", "nextHeaderIPv6", "sourceTransportPort", "destinationTransportPort",
             "icmpTypeIPv6", "icmpCodeIPv6"] + _COMMON_TAIL                             # ipfix.go:158-204


def header(length, export_time, seq, domain):
    return struct.pack(">HHIII", 10, length, export_time & 0xFFFFFFFF, seq & 0xFFFFFFFF, domain)


def template_message(v6, export_time, seq, domain=1, template_ids=(TEMPLATE_ID_V4, TEMPLATE_ID_V6)):
    """SendTemplateRecordv4 / v6: one template set (ID 2) with one template record."""
    fields = FIELDS_V6 if v6 else FIELDS_V4
    body = struct.pack(">HH", template_ids[1] if v6 else template_ids[0], len(fields))
    body += b"".join(struct.pack(">HH", _BY_NAME[f], REGISTRY[_BY_NAME[f]][2]) for f in fields)
    st = struct.pack(">HH", 2, 4 + len(body)) + body
    return header(16 + len(st), export_time, seq, domain) + st


# ---- (a) encoder

def _raw(records):
    return np.ascontiguousarray(records).view(np.uint8).reshape(-1, 144)


def _u(raw, off, nb):      # little-endian unsigned field of nb bytes at byte off, as uint64
    v = np.zeros(len(raw), dtype=np.uint64)
    for k in range(nb):
        v |= raw[:, off + k].astype(np.uint64) << np.uint64(8 * k)
    return v


def resolve_names(raw, names, unknown):
    """interfaceNamer(if_index_first_seen, lMAC) per flow (record.go:100-106) over a table of rows (if_index, mac or None,
    name bytes): the row with that index and MAC, else the first row of the index without a MAC, else `unknown`.
    Returns (n, 16) name bytes and (n,) lengths."""
    n = len(raw)
    ifx = _u(raw, 84, 4)
    lmac = np.where((raw[:, 96] == 0)[:, None], raw[:, 78:84], raw[:, 72:78])     # lMAC = dst_mac on ingress (dir 0)
    nb = np.zeros((n, 16), dtype=np.uint8)
    nl = np.full(n, len(unknown), dtype=np.int64)
    nb[:, :len(unknown)] = np.frombuffer(unknown, dtype=np.uint8)

    def fill(mask, name):
        nb[mask] = 0
        nb[mask, :len(name)] = np.frombuffer(name, dtype=np.uint8)
        nl[mask] = len(name)

    for ix, mac, name in reversed([r for r in names if r[1] is None]):           # the FIRST any-MAC row wins
        fill(ifx == ix, name)
    for ix, mac, name in reversed([r for r in names if r[1] is not None]):       # an exact (index, MAC) row wins over it
        fill((ifx == ix) & (lmac == np.frombuffer(bytes(mac), dtype=np.uint8)).all(axis=1), name)
    return nb, nl


def flow_times(ts, now_unix_ns, mono_now_ns):
    """now.Add(-Duration(mono_now - ts)) (record.go:90-97) -> (uint32(t.Unix()), uint64(t.UnixMilli())), both flooring."""
    d = (ts.astype(np.uint64) - np.uint64(mono_now_ns & (2**64 - 1))).view(np.int64)   # -(int64)(mono - ts), wrapping
    now_sec, now_nsec = divmod(now_unix_ns, 10**9)
    q, r = np.divmod(d, np.int64(10**9))
    sec = np.int64(now_sec) + q
    nsec = np.int64(now_nsec) + r
    carry = nsec >= 10**9
    sec = sec + carry
    nsec = nsec - carry * np.int64(10**9)
    ms = sec * 1000 + nsec // 1_000_000
    return sec.astype(np.uint64) & np.uint64(0xFFFFFFFF), ms.astype(np.uint64)


def _be(v, nb):            # (n,) uint64 -> (n, nb) big-endian bytes
    v = np.asarray(v, dtype=np.uint64)
    return np.stack([((v >> np.uint64(8 * (nb - 1 - k))) & np.uint64(0xFF)).astype(np.uint8) for k in range(nb)], axis=1)


def encode(records, now_unix_ns, mono_now_ns, names, export_time, seq0, unknown=b"unknown", domain=1,
           template_ids=(TEMPLATE_ID_V4, TEMPLATE_ID_V6)):
    """The messages IPFIX.ExportFlows sends for these evicted records, one per flow, message i carrying sequence number
    seq0 + i and Export Time export_time. names: rows (if_index, mac bytes or None, name bytes). Returns (bytes, offsets)."""
    raw = _raw(records)
    n = len(raw)
    eth = _u(raw, 68, 2)
    v6 = eth == 0x86DD                                                  # model.IPv6Type; anything else (0 too) is v4
    nb, nl = resolve_names(raw, names, unknown)
    length = np.where(v6, 117, 93) + nl
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(length, out=off[1:])
    out = np.zeros(int(off[-1]), dtype=np.uint8)
    t0s, t0ms = flow_times(_u(raw, 40, 8), now_unix_ns, mono_now_ns)
    t1s, t1ms = flow_times(_u(raw, 48, 8), now_unix_ns, mono_now_ns)
    seq = (np.uint64(seq0) + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    for is6 in (False, True):
        sel = np.nonzero(v6 == is6)[0]
        if len(sel) == 0:
            continue
        r = raw[sel]
        if is6:
            sip, dip = r[:, 0:16], r[:, 16:32]
        else:   # model.IP(..).To4(): bytes 12..15 of a v4-mapped address, else nil -> 0.0.0.0 (ipfix.go:264-271)
            def to4(a):
                mapped = (a[:, :10] == 0).all(axis=1) & (a[:, 10] == 0xFF) & (a[:, 11] == 0xFF)
                return np.where(mapped[:, None], a[:, 12:16], 0).astype(np.uint8)
            sip, dip = to4(r[:, 0:16]), to4(r[:, 16:32])
        cols = [
            _be(np.full(len(sel), 10), 2), _be(length[sel], 2), _be(np.full(len(sel), export_time & 0xFFFFFFFF), 4), _be(seq[sel], 4),
            _be(np.full(len(sel), domain), 4),
            _be(np.full(len(sel), template_ids[1] if is6 else template_ids[0]), 2), _be(length[sel] - 16, 2),   # set header
            _be(eth[sel], 2), r[:, 96:97],                              # ethernetType, flowDirection = direction_first_seen
            r[:, 72:78], r[:, 78:84], sip, dip,                         # MACs as stored, addresses
            r[:, 36:37],                                                # protocolIdentifier / nextHeaderIPv6 (id byte 36)
            _be(_u(r, 32, 2), 2), _be(_u(r, 34, 2), 2), r[:, 37:38], r[:, 38:39],
            _be(_u(r, 56, 8), 8), _be(_u(r, 70, 2), 2),                 # octetDeltaCount, tcpControlBits
            _be(t0s[sel], 4), _be(t0ms[sel], 8), _be(t1s[sel], 4), _be(t1ms[sel], 8),
            _be(_u(r, 64, 4), 8),                                       # packetDeltaCount = uint64(packets)
            nl[sel].astype(np.uint8)[:, None],                          # interfaceName: one length byte (ie.go:604-612)
        ]
        fixed = np.concatenate(cols, axis=1)
        assert fixed.shape[1] == (117 if is6 else 93)
        base = off[sel].astype(np.int64)
        for a in range(0, len(sel), 1 << 16):                          # scatter in slices: bounded index arrays
            out[base[a:a + (1 << 16), None] + np.arange(fixed.shape[1])] = fixed[a:a + (1 << 16)]
        for k in range(16):
            m = nl[sel] > k
            out[base[m] + fixed.shape[1] + k] = nb[sel[m], k]
    return out.tobytes(), off


# ---- (b) decoder

class Collector:
    """go-ipfix's collecting process, one message at a time (decodePacket): templates are kept per (domain, template id)."""

    def __init__(self):
        self.templates = {}

    def decode(self, msg: bytes) -> dict:
        version, length, export_time, seq, domain = struct.unpack_from(">HHIII", msg, 0)
        if version != 10:
            raise ValueError("collector only supports IPFIX (v10); invalid version %d received" % version)
        if length != len(msg):
            raise ValueError("message length %d, %d bytes received" % (length, len(msg)))
        buf = memoryview(msg)[16:]
        if len(buf) == 0:
            raise ValueError("empty IPFIX message")
        set_id, set_len = struct.unpack_from(">HH", buf, 0)
        buf = buf[4:]
        out = {"export_time": export_time, "seq": seq, "domain": domain, "set_id": set_id, "set_len": set_len}
        if set_id == 2:                                               # decodeTemplateSet: one record
            tid, count = struct.unpack_from(">HH", buf, 0)
            pos, fields = 4, []
            for _ in range(count):
                eid, elen = struct.unpack_from(">HH", buf, pos)
                pos += 4
                if eid & 0x8000:
                    raise ValueError("enterprise-specific element %d: not in this restatement" % (eid & 0x7FFF))
                name, typ, reglen = REGISTRY.get(eid, ("", "octets", elen))
                fields.append((eid, name, typ, reglen))               # the walk uses the registry's length (ie.Len)
            self.templates[(domain, tid)] = fields
            out.update(kind="template", template_id=tid, fields=[(f[0], f[3]) for f in fields])
            return out
        fields = self.templates.get((domain, set_id))
        if fields is None:
            raise ValueError("template %d with obsDomainID %d does not exist" % (set_id, domain))
        records, pos = [], 0
        while pos < len(buf):                                         # decodeDataSet
            rec = {}
            for eid, name, typ, flen in fields:
                if flen == VARLEN:                                    # getFieldLength
                    b = buf[pos]
                    pos += 1
                    if b < 255:
                        flen = b
                    else:
                        flen = struct.unpack_from(">H", buf, pos)[0]
                        pos += 2
                v = bytes(buf[pos:pos + flen])
                if len(v) < flen:
                    raise ValueError("buffer too short")
                pos += flen
                rec[name] = int.from_bytes(v, "big") if typ == "u" else (v.decode() if typ == "string" else v)
            records.append(rec)
        out.update(kind="data", records=records)
        return out
