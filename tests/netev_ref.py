"""Independent restatement of what model.NewRecord does with a SampleDecoder, for the tests (no import of the product):

  pkg/model/record.go:126-157                          the loop over the four cookies, `seen`, the injected drop
  pkg/model/flow_content.go:209-215                    addUint16
  pkg/utils/networkevents/network_events.go:17-52      causes, ToMap
  pkg/utils/networkevents/network_events.go:121-131    ToDropReasonCode
  pkg/pbflow/proto.go:140-147                          NetworkEventsMetadata (field 27)
  pkg/decode/decode_protobuf.go:184-186                the NetworkEvents key

over the numpy structs of oracle/oracle.py (NETEV, DROPS). A decoder's answers are a dict {cookie (8 bytes): event}; an event
is an ACL as the tuple (action, actor, name, namespace, direction, String()), any other event as its String() (bytes), or
None where DecodeCookie8Bytes returns an error. A cookie that is not in the dict is one the table does not know yet: it adds
nothing and is reported missing.

The JSON line is record_to_map + add_content of tests/flp_json_content_ref.py over the decorated parts plus the
NetworkEvents value; the protobuf frame is a content frame for the decorated parts (from the oracle) with the field-27
entries spliced in at their place in field-number order."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_content_ref as R  # noqa: E402
from flp_json_ref import is_deferred, jsoniter_string, marshal_sorted, record_to_map  # noqa: E402

CAUSES = R.NETWORK_EVENT_CAUSES
NO_ROW = 0xFFFF
FEAT_DROPS, FEAT_NETEV = R.FEAT["drops"], R.FEAT["network_events"]
_NETEV = struct.Struct("<QQ32s4H4H")                       # bpf/types.h:153-161: start, end, four cookies, bytes[4], packets[4]


def _b(v):
    return v.encode() if isinstance(v, str) else bytes(v)


def is_acl(ev):
    return isinstance(ev, tuple)


def event_string(ev) -> bytes:
    return _b(ev[5]) if is_acl(ev) else _b(ev)


def to_map(ev) -> dict:                                   # networkevents.ToMap
    if is_acl(ev):
        action, actor, name, namespace, direction, _ = (_b(v) for v in ev)
        return {b"Action": action, b"Type": actor, b"Feature": b"acl", b"Name": name, b"Namespace": namespace, b"Direction": direction}
    return {b"Message": _b(ev)}


def drop_cause(ev) -> int:                                # ToDropReasonCode: 0 = not a drop
    if is_acl(ev) and _b(ev[0]) == b"drop":
        actor = _b(ev[1]).decode("latin-1")
        return (1 << 24) + (CAUSES.index(actor) if actor in CAUSES else 0)
    return 0


def render_json(ev) -> bytes:
    m = to_map(ev)
    return b"{" + b",".join(jsoniter_string(k) + b":" + jsoniter_string(m[k]) for k in sorted(m)) + b"}"


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def render_pb(ev) -> bytes:
    """pbflow.NetworkEvent{Events: ToMap(ev)} as Go's deterministic marshal writes it: map entries in key order, key and
    value always present."""
    m = to_map(ev)
    out = b""
    for k in sorted(m):
        entry = b"\x0a" + _varint(len(k)) + k + b"\x12" + _varint(len(m[k])) + m[k]
        out += b"\x0a" + _varint(len(entry)) + entry
    return out


def cookie_value(c) -> int:
    return int.from_bytes(bytes(c), "little")


def table_rows(answers: dict):
    """The table's row order: cookies ascending by their little-endian 64-bit value. Returns {cookie: row}."""
    return {c: r for r, c in enumerate(sorted(answers, key=cookie_value))}


def add_u16(a, b):
    return min(a + b, 0xFFFF)


def resolve(present, netev, drops, answers: dict):
    """record.go:126-157 for every flow. present: uint8[n]; netev: NETEV[n] or None; drops: DROPS[n] or None (no flow has the
    part). Returns (present_out uint8[n], drops_out DROPS-shaped bytes [n, 32], rows uint16[n, 4], events: per flow the list
    of decoder answers in NetworkMonitorEventsMD, missing: set of cookies without an answer)."""
    n = len(present)
    rows_of = table_rows(answers)
    p_out = np.zeros(n, dtype=np.uint8)
    d_out = np.zeros((n, 32), dtype=np.uint8)
    rows = np.full((n, 4), NO_ROW, dtype=np.uint16)
    events, missing = [], set()
    dview = np.ascontiguousarray(drops).view(np.uint8).reshape(n, 32) if drops is not None else None
    nview = np.ascontiguousarray(netev).view(np.uint8).reshape(n, 72) if netev is not None else None
    for i in range(n):
        p = int(present[i])
        have = dview is not None and bool(p & FEAT_DROPS)
        d = R._DROPS.unpack(dview[i].tobytes()) if have else None
        raw = dview[i].tobytes() if have else None
        evs = []
        if nview is not None and p & FEAT_NETEV:
            start, end, cookies, *counts = _NETEV.unpack_from(nview[i].tobytes())
            seen = set()
            for k in range(4):
                by, pk = counts[k], counts[4 + k]
                if pk == 0:
                    continue
                cookie = cookies[8 * k:8 * k + 8]
                if cookie not in answers:
                    missing.add(cookie)
                    continue
                ev = answers[cookie]
                if ev is None:                            # err != nil
                    continue
                s = event_string(ev)
                if s not in seen:
                    seen.add(s)
                    rows[i, len(evs)] = rows_of[cookie]
                    evs.append(ev)
                cause = drop_cause(ev)
                if cause:
                    if d is None:
                        d = [start, end, by, pk, cause, 0, 0, 0]
                        raw = None
                    else:
                        d = list(d)
                        d[4], d[2], d[3] = cause, add_u16(d[2], by), add_u16(d[3], pk)
                        # the struct's padding travels with it: only the three fields change
                        raw = raw[:16] + R._DROPS.pack(*d)[16:24] + raw[24:] if raw is not None else None
        if d is not None:
            d_out[i] = np.frombuffer(raw if raw is not None else R._DROPS.pack(*d), dtype=np.uint8)
        p_out[i] = (p & ~FEAT_DROPS) | (FEAT_DROPS if d is not None else 0)
        events.append(evs)
    return p_out, d_out, rows, events, missing


def resolve_loop(present, netev, drops, decoder):
    """The shim's protocol: resolve, ask the decoder about the missing cookies, resolve again. Returns resolve()'s result, the
    answers and the number of decoder calls."""
    answers, calls = {}, 0
    while True:
        out = resolve(present, netev, drops, answers)
        if not out[4]:
            return out, answers, calls
        for c in sorted(out[4]):
            answers[c] = decoder(c)
            calls += 1


def encode_json(records, present_out, parts, events, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown=b"unknown"):
    """The lines, as flp_json_content_ref.encode gives them, with the NetworkEvents key of the flows that have events.
    parts["drops"] is resolve()'s drops_out."""
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1, 144)
    n = len(raw)
    off = np.zeros(n + 1, dtype=np.uint64)
    deferred = np.zeros(n, dtype=np.uint8)
    memo, lines, pos = {}, [], 0
    for i in range(n):
        rec = raw[i].tobytes()
        if is_deferred(rec):
            deferred[i] = 1
        else:
            m = R.add_content(record_to_map(rec, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown, memo),
                              R.flow_parts(present_out, parts, i))
            body = marshal_sorted(m)
            if events[i]:                                 # spliced in as rendered: a list of maps is not a _value of flp_json_ref
                keys = sorted(list(m) + [b"NetworkEvents"])
                at = keys.index(b"NetworkEvents")
                val = b'"NetworkEvents":[' + b",".join(render_json(e) for e in events[i]) + b"]"
                head = marshal_sorted({k: m[k] for k in keys[:at]})[:-1]
                tail = marshal_sorted({k: m[k] for k in keys[at + 1:]})[1:]
                body = head + (b"," if at else b"") + val + (b"," if len(tail) > 1 else b"") + tail
            lines.append(body + b"\n")
            pos += len(lines[-1])
        off[i + 1] = pos
    return b"".join(lines), off, deferred


def _read_varint(b, i):
    v = s = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            return v, i


def splice_field27(body: bytes, events) -> bytes:
    """A serialized pbflow.Record with one network_events_metadata entry per event at its place in field-number order."""
    if not events:
        return body
    ins = b"".join(b"\xda\x01" + _varint(len(render_pb(e))) + render_pb(e) for e in events)
    i = 0
    while i < len(body):
        tag, j = _read_varint(body, i)
        if tag >> 3 > 27:
            break
        wt = tag & 7
        if wt == 0:
            _, j = _read_varint(body, j)
        elif wt == 2:
            ln, j = _read_varint(body, j)
            j += ln
        elif wt == 5:
            j += 4
        elif wt == 1:
            j += 8
        else:
            raise ValueError("wire type %d" % wt)
        i = j
    return body[:i] + ins + body[i:]


def encode_pb(O, records, present_out, parts, events, now_unix_ns, mono_now_ns, agent_ip16, names_rows, unknown=b"unknown"):
    """(bytes, frame offsets uint64[n + 1], body lengths uint32[n]): the oracle's content frame of every flow over the decorated
    parts, field 27 spliced in, the frame's length written again. names_rows: (if_index, mac, name str, udn str) rows."""
    recs = np.ascontiguousarray(records).view(O.FLOW_RECORD)
    n = len(recs)
    c = np.zeros(n, dtype=O.CONTENT)
    c["base"] = recs["metrics"]
    for kind, has in (("additional", "has_additional"), ("dns", "has_dns"), ("drops", "has_drops"), ("xlat", "has_xlat"), ("quic", "has_quic")):
        a = (parts or {}).get(kind)
        if a is None:
            continue
        c[has] = (np.asarray(present_out) & R.FEAT[kind]) != 0
        c[kind] = np.ascontiguousarray(a).view(np.uint8).reshape(n, -1).copy().view(O.KIND_DTYPES[O.KIND_INDEX[kind]]).reshape(n)
    bodies = O.pb_encode_contents(recs["id"], c, O.pb_options(now_unix_ns, mono_now_ns, agent_ip16, O.intf_table(names_rows), unknown))
    off = np.zeros(n + 1, dtype=np.uint64)
    blen = np.zeros(n, dtype=np.uint32)
    out = []
    for i in range(n):
        body = splice_field27(bodies[i], events[i])
        blen[i] = len(body)
        out.append(b"\x0a" + _varint(len(body)) + body)
        off[i + 1] = off[i] + len(out[-1])
    return b"".join(out), off, blen
