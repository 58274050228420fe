"""Independent restatement of flowlogs-pipeline's `write loki` stage and of loki-client-go's batching and wire format over the
maps of tests/flp_json_net_ref.py, for the tests (no import of the product). Paths under the reference's vendor/:

  netobserv/flowlogs-pipeline/pkg/pipeline/write/write_loki.go:223-251   splitLabelsLines
  .../write_loki.go:253-277, 279-299                                     extractTimestamp, getFloat64
  .../write_stdout.go:42-51                                              formatter("json"): the marshalled map, no newline
  netobserv/loki-client-go/loki/client.go:154-172                        a batch is sent when bytes + len(line) > BatchSize
  netobserv/loki-client-go/loki/batch.go:39-54, 63-65, 96-107            streams of a batch by LabelSet.String(), bytes = line bytes
  netobserv/loki-client-go/pkg/logproto/types.go:88-144                  PushRequest, Stream, Entry MarshalTo
  netobserv/loki-client-go/pkg/logproto/timestamp.go:31-36, 59-106       validateTimestamp, the Timestamp's fields
  prometheus/common/model/labelset_string.go:23-43                       LabelSet.String()

Streams are ordered by the first flow of the call that belongs to them (Go's map order is any order). A flow whose timestamp
fails validateTimestamp, or whose float64 product leaves int64, is reported as deferred and takes part in no batch: the
reference would lose that flow's whole batch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_net_ref as R  # noqa: E402
import flp_json_tls_ref as RT  # noqa: E402
import flp_json_content_ref as RC  # noqa: E402
import netev_ref as RN  # noqa: E402
from flp_json_ref import _value, jsoniter_string, record_to_map  # noqa: E402

MIN_SECONDS, MAX_SECONDS = -62135596800, 253402300800


def _b(v) -> bytes:
    return v.encode() if isinstance(v, str) else bytes(v)


class Raw:
    """A value that is already JSON text: the rendered NetworkEvents list."""

    def __init__(self, raw: bytes):
        self.raw = raw


def marshal_sorted(m: dict) -> bytes:
    """jsoniter's sorted-keys marshal of a line map (flp_json_ref.marshal_sorted, with Raw values written as they are)."""
    return b"{" + b",".join(jsoniter_string(k) + b":" + (m[k].raw if isinstance(m[k], Raw) else _value(m[k])) for k in sorted(m)) + b"}"


def flow_maps(records, names_tls, table, layer, rules, now_unix_ns, mono_now_ns, names, agent_ip, time_received, hash_ids=None, present=None, parts=None,
              events=None):
    """One enriched map per flow as the stage sees it; None for a flow extract conntrack does not pass on (hash_ids given).
    present / parts: the feature parts of full flow contents; events[i]: the flow's decoded network events (netev_ref)."""
    import numpy as np
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1, 144)
    cats = R.parse_subnets(rules["labels"]) if rules.get("labels") is not None else []
    memo, out = {}, []
    for i in range(len(raw)):
        rec = raw[i].tobytes()
        m = RT.add_tls(record_to_map(rec, now_unix_ns, mono_now_ns, names, agent_ip, time_received, b"unknown", memo), rec, names_tls)
        if present is not None:
            RC.add_content(m, RC.flow_parts(present, parts, i))
        R.apply_rules(m, table, layer, rules, cats)
        if events is not None and events[i]:
            m[b"NetworkEvents"] = Raw(b"[" + b",".join(RN.render_json(e) for e in events[i]) + b"]")
        if hash_ids is not None:
            if b"SrcPort" not in m:                        # the stage's filter: the flows that have ports
                out.append(None)
                continue
            m[b"_HashId"] = b"%x" % int(hash_ids[i])
            m[b"_RecordType"] = b"flowLog"
        out.append(m)
    return out


def utf8_valid(v: bytes) -> bool:
    try:
        v.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def convert_to_string(v) -> bytes:
    return b"%d" % v if isinstance(v, int) else bytes(v)


def split_labels_lines(m: dict, sane_labels: dict, ignore, static_labels: dict):
    """(labels {name bytes: value bytes}, the line's map)."""
    labels = {_b(k): _b(v) for k, v in static_labels.items()}
    lines = {}
    for k, v in m.items():
        if k in ignore:
            continue
        if k in sane_labels:
            lv = convert_to_string(v)
            if not utf8_valid(lv):
                continue
            labels[_b(sane_labels[k])] = lv
        else:
            lines[k] = v
    return labels, lines


def go_quote(v: bytes) -> bytes:
    """strconv.Quote of ASCII text."""
    short = {7: b"\\a", 8: b"\\b", 12: b"\\f", 10: b"\\n", 13: b"\\r", 9: b"\\t", 11: b"\\v", 34: b'\\"', 92: b"\\\\"}
    out = b'"'
    for c in v:
        assert c < 0x80, "ASCII only"
        out += short[c] if c in short else b"\\x%02x" % c if c < 32 or c == 127 else bytes([c])
    return out + b'"'


def labelset_string(labels: dict) -> bytes:
    return b"{" + b", ".join(k + b"=" + go_quote(labels[k]) for k in sorted(labels)) + b"}"


def extract_timestamp(lines: dict, label: bytes, scale: float, now_unix_ns: int):
    """(seconds, nanos) of the time.Time, or None where int64(float64) is not defined."""
    v = lines.get(label) if label else None
    if v is None or not isinstance(v, int) or float(v) == 0.0:
        tn = now_unix_ns
    else:
        prod = float(v) * scale
        if not (-9223372036854775808.0 <= prod < 9223372036854775808.0):
            return None
        tn = int(prod)
    q = abs(tn) // 10 ** 9 * (1 if tn >= 0 else -1)               # Go's / and % truncate towards zero
    sec, nsec = q, tn - q * 10 ** 9
    if nsec < 0:                                                  # time.Unix
        sec, nsec = sec - 1, nsec + 10 ** 9
    return sec, nsec


def varint(v: int) -> bytes:
    v &= (1 << 64) - 1
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def marshal_timestamp(sec: int, nsec: int) -> bytes:
    return (b"\x08" + varint(sec) if sec else b"") + (b"\x10" + varint(nsec) if nsec else b"")


def marshal_entry(sec: int, nsec: int, line: bytes) -> bytes:
    ts = marshal_timestamp(sec, nsec)
    return b"\x0a" + varint(len(ts)) + ts + (b"\x12" + varint(len(line)) + line if line else b"")


def marshal_stream(labels: bytes, entries) -> bytes:
    out = b"\x0a" + varint(len(labels)) + labels if labels else b""
    for e in entries:
        body = marshal_entry(*e)
        out += b"\x12" + varint(len(body)) + body
    return out


def marshal_push_request(streams) -> bytes:
    """streams: [(labels text, [(sec, nsec, line)])] in request order."""
    out = b""
    for labels, entries in streams:
        body = marshal_stream(labels, entries)
        out += b"\x0a" + varint(len(body)) + body
    return out


def write_loki(maps, sane_labels, ignore, static_labels, timestamp_label, scale, batch_size, now_unix_ns):
    """The stage over one call's maps. Returns (bodies, batches, deferred): bodies[b] the PushRequest of batch b with its streams
    in order of their first flow in the CALL; batches[b] = [(labels text, [(sec, nsec, line)])] in that order; deferred: flow
    indexes."""
    sane = {_b(k): v for k, v in sane_labels.items()}
    ign = {_b(k) for k in ignore}
    order, batches, deferred = {}, [], []
    cur, cur_bytes = None, 0
    for i, m in enumerate(maps):
        if m is None:
            continue
        labels, lines = split_labels_lines(m, sane, ign, static_labels)
        line = marshal_sorted(lines)
        t = extract_timestamp(lines, _b(timestamp_label), scale, now_unix_ns)
        if t is None or not (MIN_SECONDS <= t[0] < MAX_SECONDS):
            deferred.append(i)
            continue
        text = labelset_string(labels)
        order.setdefault(text, len(order))
        if cur is not None and cur_bytes + len(line) > batch_size:   # client.go:161: strictly greater
            batches.append(cur)
            cur, cur_bytes = None, 0
        if cur is None:
            cur = {}
        cur.setdefault(text, []).append((t[0], t[1], line))
        cur_bytes += len(line)
    if cur is not None:
        batches.append(cur)
    ordered = [[(text, b[text]) for text in sorted(b, key=order.get)] for b in batches]
    return [marshal_push_request(b) for b in ordered], ordered, deferred
