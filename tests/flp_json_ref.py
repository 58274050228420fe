"""Independent restatement of the reference's direct-FLP stdout path, for the tests (no import of the product, no
json.dumps, no ipaddress):

  pkg/model/record.go:82-114              NewRecord: flow times, lMAC, the interface list
  pkg/model/record.go:167-183             NewIntfDirUdn (here: the UDN column of the namer table)
  pkg/decode/decode_protobuf.go:57-127    RecordToMap, the keys of a record that carries only BpfFlowMetrics
  pkg/model/tls_types.go                  the TLSTypes name list
  Go net.IP.String / netip appendTo6, net.HardwareAddr.String, time.Time.Add / UnixMilli
  json-iterator stream_str.go:311-372     WriteString (no HTML escaping) and its safeSet
  json-iterator reflect_map.go            sortKeysMapEncoder: keys in byte order; reflect_slice.go: a nil slice is null
  flowlogs-pipeline write_stdout.go:37-51 one marshalled map per line

Strings are bytes throughout: interface names and UDNs are arbitrary bytes and jsoniter copies bytes from 0x80 up as
they are. A record with ssl_version, tls_cipher_suite or tls_key_share set is deferred (crypto/tls names are not
restated): empty line, deferred flag."""
import struct

import numpy as np

M64 = (1 << 64) - 1
_KEY = struct.Struct("<16s16sHHBBBx")
_METRICS = struct.Struct("<QQQIHH6s6sIIIBBBB6s2x6IHHHBB4x")
assert _KEY.size == 40 and _METRICS.size == 104
TLS_TYPES = [(1, b"ClientHello"), (2, b"ServerHello"), (4, b"OtherHandshake"), (8, b"ChangeCipher"), (16, b"Alert"), (32, b"AppData")]
_HEX = b"0123456789abcdef"


def _i64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def go_mac(b: bytes) -> bytes:                 # net.HardwareAddr.String(): hex pairs joined by ':'
    out = bytearray()
    for k, x in enumerate(b):
        if k:
            out += b":"
        out.append(_HEX[x >> 4])
        out.append(_HEX[x & 15])
    return bytes(out)


def go_ip(b) -> bytes:
    """net.IP.String(): nil -> "<nil>"; a 16-byte address that To4() accepts (ten zero bytes, ff ff) -> dotted quad;
    otherwise netip.Addr.appendTo6: the first longest run of two or more zero groups -> "::", lower-case hex groups."""
    if b is None or len(b) == 0:
        return b"<nil>"
    if len(b) == 4:
        b = bytes(10) + b"\xff\xff" + bytes(b)
    assert len(b) == 16
    if b[:10] == bytes(10) and b[10] == 0xFF and b[11] == 0xFF:
        return b".".join(str(x).encode() for x in b[12:])
    g = [(b[2 * k] << 8) | b[2 * k + 1] for k in range(8)]
    z0, z1 = 255, 255
    i = 0
    while i < 8:                                # appendTo6's search, as written there
        j = i
        while j < 8 and g[j] == 0:
            j += 1
        if j - i >= 2 and j - i > z1 - z0:
            z0, z1 = i, j
        i += 1
    out = bytearray()
    i = 0
    while i < 8:
        if i == z0:
            out += b"::"
            i = z1
            if i >= 8:
                break
        elif i > 0:
            out += b":"
        out += b"%x" % g[i]
        i += 1
    return bytes(out)


def jsoniter_string(s: bytes) -> bytes:
    """Stream.WriteString: quotes; \\" \\\\ \\n \\r \\t; other bytes below 0x20 as \\u00xx; everything else (0x7f and bytes from
    0x80 up included) copied."""
    out = bytearray(b'"')
    for c in s:
        if c > 31 and c != 0x22 and c != 0x5C:
            out.append(c)
        elif c in (0x22, 0x5C):
            out += bytes([0x5C, c])
        elif c == 0x0A:
            out += b"\\n"
        elif c == 0x0D:
            out += b"\\r"
        elif c == 0x09:
            out += b"\\t"
        else:
            out += b"\\u00" + bytes([_HEX[c >> 4], _HEX[c & 15]])
    out += b'"'
    return bytes(out)


def unix_milli(now_unix_ns: int, mono_now_ns: int, ts: int) -> int:
    """currentTime.Add(-time.Duration(mono - ts)).UnixMilli() with Go's wrapping integer arithmetic."""
    d = _i64(-_i64(mono_now_ns - ts))
    sec, nsec = divmod(now_unix_ns, 10**9)                   # time.Unix(0, ns): 0 <= nsec < 1e9
    q = abs(d) // 10**9 * (1 if d >= 0 else -1)              # Go's / and % truncate towards zero
    sec, nsec = sec + q, nsec + (d - q * 10**9)
    if nsec >= 10**9:
        sec, nsec = sec + 1, nsec - 10**9
    elif nsec < 0:
        sec, nsec = sec - 1, nsec + 10**9
    return _i64(sec * 1000 + nsec // 10**6)


def lookup(names, if_index: int, mac: bytes, unknown: bytes):
    """The namer table's rule: the row with this index and MAC, else the first row of the index without a MAC, else the
    unknown name and no UDN. names: rows (if_index, mac or None, name bytes, udn bytes)."""
    for ix, m, name, udn in names:
        if ix == if_index and m is not None and bytes(m) == mac:
            return name, udn
    for ix, m, name, udn in names:
        if ix == if_index and m is None:
            return name, udn
    return unknown, b""


def is_deferred(rec: bytes) -> bool:
    m = _METRICS.unpack_from(rec, 40)
    return bool(m[22] or m[23] or m[24])         # ssl_version, tls_cipher_suite, tls_key_share


def record_to_map(rec: bytes, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown=b"unknown", _memo=None):
    """RecordToMap(NewRecord(...)) for one 144-byte record: {key bytes: int | bytes | list | None}."""
    sip, dip, sport, dport, proto, icmp_type, icmp_code = _KEY.unpack_from(rec, 0)
    (start, end, nbytes, packets, eth, flags, smac, dmac, ifx, _lock, sampling, direction, _errno, dscp, nb_obs, odir,
     oi0, oi1, oi2, oi3, oi4, oi5, _ssl, _cipher, _share, tls_types, _misc) = _METRICS.unpack_from(rec, 40)
    lmac = dmac if direction == 0 else smac
    intfs = [(ifx, direction)] + [((oi0, oi1, oi2, oi3, oi4, oi5)[k], odir[k]) for k in range(min(nb_obs, 6))]
    memo = _memo if _memo is not None else {}
    named = []
    for ix, _ in intfs:
        k = (ix, lmac)
        if k not in memo:
            memo[k] = lookup(names, ix, lmac, unknown)
        named.append(memo[k])
    out = {
        b"SrcMac": go_mac(smac), b"DstMac": go_mac(dmac), b"Etype": eth,
        b"TimeFlowStartMs": unix_milli(now_unix_ns, mono_now_ns, start), b"TimeFlowEndMs": unix_milli(now_unix_ns, mono_now_ns, end),
        b"TimeReceived": time_received, b"AgentIP": go_ip(agent_ip),
        b"IfDirections": [d for _, d in intfs], b"Interfaces": [n for n, _ in named], b"Udns": [u for _, u in named],
    }
    if nbytes:
        out[b"Bytes"] = nbytes
    if packets:
        out[b"Packets"] = packets
    if sampling:
        out[b"Sampling"] = sampling
    if tls_types > 0:
        v = [name for bit, name in TLS_TYPES if tls_types & bit]
        out[b"TLSTypes"] = v if v else None                   # append to a nil slice never ran: nil
    if eth in (0x0800, 0x86DD):
        out[b"SrcAddr"], out[b"DstAddr"], out[b"Proto"], out[b"Dscp"] = go_ip(sip), go_ip(dip), proto, dscp
        if proto in (1, 58):
            out[b"IcmpType"], out[b"IcmpCode"] = icmp_type, icmp_code
        elif proto in (6, 17, 132):
            out[b"SrcPort"], out[b"DstPort"] = sport, dport
            if proto == 6:
                out[b"Flags"] = flags
    return out


def _value(v) -> bytes:
    if v is None:
        return b"null"
    if isinstance(v, (bytes, bytearray)):
        return jsoniter_string(bytes(v))
    if isinstance(v, list):
        return b"[" + b",".join(_value(x) for x in v) + b"]"
    return str(int(v)).encode()


def marshal_sorted(m: dict) -> bytes:
    """jsoniter.Config{SortMapKeys: true}.Marshal of a map[string]interface{}: keys in byte order, no spaces."""
    return b"{" + b",".join(jsoniter_string(k) + b":" + _value(m[k]) for k in sorted(m)) + b"}"


def encode(records, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown=b"unknown"):
    """The lines of these evicted records. names: rows (if_index, mac or None, name bytes, udn bytes); agent_ip: bytes or
    None. Returns (bytes, offsets uint64[n + 1], deferred uint8[n])."""
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1, 144)
    n = len(raw)
    blob = raw.tobytes()
    off = np.zeros(n + 1, dtype=np.uint64)
    deferred = np.zeros(n, dtype=np.uint8)
    memo, parts, pos = {}, [], 0
    for i in range(n):
        rec = blob[144 * i:144 * i + 144]
        if is_deferred(rec):
            deferred[i] = 1
        else:
            line = marshal_sorted(record_to_map(rec, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown, memo)) + b"\n"
            parts.append(line)
            pos += len(line)
        off[i + 1] = pos
    return b"".join(parts), off, deferred
