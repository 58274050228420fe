"""flowlogs-pipeline's `extract conntrack` over the device's per-call fold (include/nfagg.h, "Conversation tracking").

FlowTable.conn_fold does what is per flow and order-free: the filter, the three gob + FNV-64a hashes, the GROUP BY connection,
the sums, the least start and the greatest end. ConnTrack visits the CONNECTIONS of a call, in the order of their first flow,
and keeps what depends on order and on the clock: the store with its two ordered lists per scheduling group and phase
(store.go), the timeouts, maxConnectionsTracked, and the newConnection / heartbeat / endConnection records (conntrack.go
66-180). Three positions per connection make that exact without seeing the flows:

  first_idx      who creates the connection, in which order connections are admitted while the store has room (the store
                 only grows inside Extract's loop), where the newConnection record goes, the order of the heartbeat list;
  last_idx       an active connection moves to the back of its expiry list with every flow: the list's order is that of the
                 last flows;
  first_fin_idx  with detectEndConnection the first FIN moves the connection to the terminating list, and nothing moves it
                 afterwards: the terminating list's order is that of the first FINs.

Differences from the reference, by design: one `now` per call; aggregates are exact integers in the store and become
float64 on output; two endpoint pairs whose 64-bit totals collide are one connection (as in the reference's store) and only
their AB / BA split may differ.

Served here: the key definition NetObserv's operator generates (src = [SrcAddr, SrcPort], dst = [DstAddr, DstPort], common =
[Proto], hash over [common], A = src, B = dst); `count`; `sum` over Bytes or Packets; `min` over TimeFlowStartMs and `max`
over TimeFlowEndMs, not split (the partial carries one least start and one greatest end); `first` / `last` over a key
RecordToMap always writes and that needs no table: FIRST_LAST_FIELDS. Everything else Validate accepts raises ValueError.

Output: apply / extract return the records as dicts. conversations returns the conversation records as the two arrays of
FlowTable.encode_conn_json, extract_lines the stage's whole output as the bytes of its JSON lines, encoded on the device."""
import json
import re

import numpy as np

from . import _lib as L
from .records import FLOW_RECORD

KEY_DEFINITION = {"fieldGroups": [{"name": "src", "fields": ["SrcAddr", "SrcPort"]}, {"name": "dst", "fields": ["DstAddr", "DstPort"]},
                                  {"name": "common", "fields": ["Proto"]}],
                  "hash": {"fieldGroupRefs": ["common"], "fieldGroupARef": "src", "fieldGroupBRef": "dst"}}
KEY_FIELDS = ("SrcAddr", "SrcPort", "DstAddr", "DstPort", "Proto")
FIRST_LAST_FIELDS = KEY_FIELDS + ("SrcMac", "DstMac", "Etype", "Dscp", "TimeFlowStartMs", "TimeFlowEndMs", "IfDirections")
RECORD_TYPES = ("newConnection", "endConnection", "heartbeat", "flowLog")
FIN, SYN_ACK = 0x01, 0x100
_UNITS = {"ns": 1, "us": 10**3, "µs": 10**3, "μs": 10**3, "ms": 10**6, "s": 10**9, "m": 60 * 10**9, "h": 3600 * 10**9}
_M64 = (1 << 64) - 1


def parse_duration(v) -> int:
    """A Go duration string ("1m30s", "500ms") or a number of nanoseconds -> nanoseconds."""
    if isinstance(v, (int, float)):
        return int(v)
    if v in ("0", "", None):
        return 0
    parts = re.findall(r"([0-9]*\.?[0-9]+)(ns|us|µs|μs|ms|s|m|h)", v)
    if not parts or "".join(a + b for a, b in parts) != v.lstrip("+"):
        raise ValueError("invalid duration %r" % (v,))
    return sum(int(round(float(a) * _UNITS[u])) for a, u in parts)


def _validate(cfg: dict) -> None:
    """api/conntrack.go:105-229, its errors in its order."""
    kd = cfg.get("keyDefinition", {})
    hd = kd.get("hash", {})
    a_ref, b_ref = hd.get("fieldGroupARef", ""), hd.get("fieldGroupBRef", "")
    if (a_ref == "") != (b_ref == ""):
        raise ValueError("only one of 'fieldGroupARef' and 'fieldGroupBRef' is set. They should both be set or both unset")
    bidi = a_ref != ""
    fields = cfg.get("outputFields", [])
    for of in fields:
        op, split = of.get("operation", ""), of.get("splitAB", False)
        if split and not bidi:
            raise ValueError("output field %r has splitAB=true although bidirection is not enabled (fieldGroupARef is empty)" % of.get("name", ""))
        if op not in ("sum", "count", "min", "max", "first", "last") or (op in ("first", "last") and split):
            raise ValueError("unknown operation %r in output field %r" % (op, of.get("name", "")))
    seen = set()
    for of in fields:
        name = of.get("name", "")
        for f in ((name + "_AB", name + "_BA") if of.get("splitAB", False) else (name,)):
            if f in seen:
                raise ValueError("duplicate outputField %r" % f)
            seen.add(f)
    groups = set()
    for fg in kd.get("fieldGroups", []):
        if fg.get("name", "") in groups:
            raise ValueError("duplicate fieldGroup %r" % fg.get("name", ""))
        groups.add(fg.get("name", ""))
    if bidi and a_ref not in groups:
        raise ValueError("undefined fieldGroupARef %r" % a_ref)
    if bidi and b_ref not in groups:
        raise ValueError("undefined fieldGroupBRef %r" % b_ref)
    for ref in hd.get("fieldGroupRefs", []):
        if ref not in groups:
            raise ValueError("undefined fieldGroup %r" % ref)
    for ort in cfg.get("outputRecordTypes", []):
        if ort not in RECORD_TYPES:
            raise ValueError("undefined output record type %r" % ort)
    keys = {k for fg in kd.get("fieldGroups", []) for k in fg.get("fields", [])}
    sched = cfg.get("scheduling", [])
    for i, g in enumerate(sched):
        for k in g.get("selector", None) or {}:
            if k not in keys:
                raise ValueError("selector key %r in scheduling group %d is not defined in the keys" % (k, i))
    n_default = 0
    for i, g in enumerate(sched):
        if not (g.get("selector", None) or {}):
            n_default += 1
            if i != len(sched) - 1:
                raise ValueError("scheduling group %d has a default selector but is not the last scheduling group" % i)
    if n_default != 1:
        raise ValueError("found %d default selectors. There should be exactly 1" % n_default)
    tf = cfg.get("tcpFlags", {})
    if not tf.get("fieldName", "") and (tf.get("detectEndConnection", False) or tf.get("swapAB", False)):
        raise ValueError("TCPFlags.FieldName is empty although DetectEndConnection or SwapAB are enabled")
    if tf.get("swapAB", False) and not bidi:
        raise ValueError("SwapAB is enabled although bidirection is not enabled (fieldGroupARef is empty)")
    by_name = {fg.get("name", ""): fg.get("fields", []) for fg in kd.get("fieldGroups", [])}
    fa, fb = (by_name.get(a_ref, []), by_name.get(b_ref, [])) if bidi else ([], [])
    if len(fa) != len(fb):
        raise ValueError("mismatch between the field count of fieldGroupARef %d and fieldGroupBRef %d" % (len(fa), len(fb)))


def _served(cfg: dict) -> None:
    """What Validate accepts and this path does not serve."""
    kd = cfg.get("keyDefinition", {})
    got = ([(fg.get("name"), list(fg.get("fields", []))) for fg in kd.get("fieldGroups", [])], list(kd.get("hash", {}).get("fieldGroupRefs", [])),
           kd.get("hash", {}).get("fieldGroupARef", ""), kd.get("hash", {}).get("fieldGroupBRef", ""))
    want = ([(fg["name"], fg["fields"]) for fg in KEY_DEFINITION["fieldGroups"]], ["common"], "src", "dst")
    if got != want:
        raise ValueError("the device fold serves one key definition: src = [SrcAddr, SrcPort], dst = [DstAddr, DstPort], common = [Proto], "
                         "hash over [common], A = src, B = dst")
    tf = cfg.get("tcpFlags", {})
    if (tf.get("detectEndConnection", False) or tf.get("swapAB", False)) and tf.get("fieldName", "") != "Flags":
        raise ValueError("tcpFlags.fieldName %r: the device fold reads the record's Flags" % tf.get("fieldName", ""))
    for of in cfg.get("outputFields", []):
        op, name = of["operation"], of.get("name", "")
        if not name:
            raise ValueError("empty name %r" % (of,))
        inp = of.get("input", "") or name
        if op == "sum" and inp not in ("Bytes", "Packets"):
            raise ValueError("output field %r: sum over %r is not served (Bytes, Packets)" % (name, inp))
        if op == "min" and (inp != "TimeFlowStartMs" or of.get("splitAB", False)):
            raise ValueError("output field %r: min is served over TimeFlowStartMs, not split" % name)
        if op == "max" and (inp != "TimeFlowEndMs" or of.get("splitAB", False)):
            raise ValueError("output field %r: max is served over TimeFlowEndMs, not split" % name)
        if op in ("first", "last") and inp not in FIRST_LAST_FIELDS:
            raise ValueError("output field %r: %s over %r, a key RecordToMap does not always write or that needs a table" % (name, op, inp))
        if of.get("reportMissing", False) and op in ("sum", "min", "max") and inp in ("Bytes", "Packets"):
            raise ValueError("output field %r: reportMissing on %r, which RecordToMap omits when zero" % (name, inp))


def go_ip(b: bytes) -> str:
    """net.IP.String() of a 16-byte address: the dotted quad for a v4-mapped one, else netip's appendTo6."""
    b = bytes(b)
    if b[:12] == bytes(10) + b"\xff\xff":
        return "%d.%d.%d.%d" % tuple(b[12:])
    g = [(b[2 * k] << 8) | b[2 * k + 1] for k in range(8)]
    z0, zlen = -1, 1
    for k in range(8):
        j = k
        while j < 8 and g[j] == 0:
            j += 1
        if j - k > zlen:
            z0, zlen = k, j - k
    if z0 < 0:
        return ":".join("%x" % x for x in g)
    return ":".join("%x" % x for x in g[:z0]) + "::" + ":".join("%x" % x for x in g[z0 + zlen:])


def unix_milli(now_unix_ns: int, mono_now_ns: int, ts: int) -> int:
    """currentTime.Add(-Duration(mono - ts)).UnixMilli() (record.go:90-97) with Go's wrapping arithmetic."""
    def i64(v):
        v &= _M64
        return v - (1 << 64) if v >> 63 else v
    d = i64(-i64(mono_now_ns - ts))
    sec, nsec = divmod(now_unix_ns, 10**9)
    q = abs(d) // 10**9 * (1 if d >= 0 else -1)
    sec, nsec = sec + q, nsec + (d - q * 10**9)
    if nsec >= 10**9:
        sec, nsec = sec + 1, nsec - 10**9
    elif nsec < 0:
        sec, nsec = sec - 1, nsec + 10**9
    return i64(sec * 1000 + nsec // 10**6)


def _text(v) -> str:                    # conn.go:127-178: a key and a selector value compare as text
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, float) and v == int(v):
        v = int(v)
    return str(v)


class _Conn:
    __slots__ = ("hash_a", "hash_total", "keys", "flows", "bytes", "packets", "start_min", "end_max", "first", "last", "expiry", "next_heartbeat", "reported",
                 "carrier", "snap_first", "snap_last")


class _Lists:
    """utils.MultiOrderedMap for the store's two orders: dicts keep insertion order, a move to the back is pop and insert."""
    def __init__(self):
        self.rec, self.expiry, self.heartbeat = {}, {}, {}

    def add(self, h, c):
        self.rec[h] = c
        self.expiry[h] = self.heartbeat[h] = None

    def remove(self, h):
        del self.rec[h], self.expiry[h], self.heartbeat[h]


class ConnTrack:
    """ConnTrack(config): FLP's ConnTrack parameters as a dict or JSON text. extract() is Extract for one call's records."""

    def __init__(self, config):
        cfg = json.loads(config) if isinstance(config, (str, bytes)) else dict(config)
        _validate(cfg)
        _served(cfg)
        self.config = cfg
        tf = cfg.get("tcpFlags", {})
        self.detect_end, self.swap_ab = bool(tf.get("detectEndConnection", False)), bool(tf.get("swapAB", False))
        self.max_conns = int(cfg.get("maxConnectionsTracked", 0))
        self.out_types = set(cfg.get("outputRecordTypes", []))
        self.fields = [dict(op=of["operation"], name=of["name"], inp=of.get("input", "") or of["name"], split=bool(of.get("splitAB", False)))
                       for of in cfg.get("outputFields", [])]
        self.groups = [dict(selector=g.get("selector", None) or {}, end=parse_duration(g.get("endConnectionTimeout", 0)),
                            term=parse_duration(g.get("terminatingTimeout", 0)), hb=parse_duration(g.get("heartbeatInterval", 0)),
                            active=_Lists(), terminating=_Lists()) for g in cfg.get("scheduling", [])]
        self.group_of = {}              # hashID2groupIdx
        self.now = 0

    def __len__(self):
        return len(self.group_of)

    def layout(self, table=None):
        """The stage's outputFields as a table.ConnLayout for FlowTable.encode_conn_json: on table's device, or checked on the host
        alone with table=None."""
        from .table import ConnLayout
        return ConnLayout([dict(name=f["name"], operation=f["op"], input=f["inp"], splitAB=f["split"]) for f in self.fields], table)

    # ---- a record's values, as RecordToMap writes them
    @staticmethod
    def _field(rec, name, now_unix_ns, mono_now_ns):
        k, m = rec["id"], rec["metrics"]
        if name == "SrcAddr":
            return go_ip(k["src_ip"].tobytes())
        if name == "DstAddr":
            return go_ip(k["dst_ip"].tobytes())
        if name in ("SrcPort", "DstPort"):
            return int(k["src_port" if name == "SrcPort" else "dst_port"])
        if name == "Proto":
            return int(k["transport_protocol"])
        if name in ("SrcMac", "DstMac"):
            return ":".join("%02x" % x for x in m["src_mac" if name == "SrcMac" else "dst_mac"].tobytes())
        if name == "Etype":
            return int(m["eth_protocol"])
        if name == "Dscp":
            return int(m["dscp"])
        if name == "TimeFlowStartMs":
            return unix_milli(now_unix_ns, mono_now_ns, int(m["start_mono_time_ts"]))
        if name == "TimeFlowEndMs":
            return unix_milli(now_unix_ns, mono_now_ns, int(m["end_mono_time_ts"]))
        if name == "IfDirections":      # record.go:100-114: the first-seen direction, then the observed ones
            return [int(m["direction_first_seen"])] + [int(x) for x in m["observed_direction"][:min(int(m["nb_observed_intf"]), 6)]]
        raise KeyError(name)

    def _to_map(self, c) -> dict:       # conn.go:101-114: a zero float and a nil are omitted, the keys prevail
        gm = {}
        for f in self.fields:
            op = f["op"]
            if op in ("first", "last"):
                v = (c.first if op == "first" else c.last).get(f["name"])
                if v is not None:
                    gm[f["name"]] = v
                continue
            if op == "min":
                vals = [(f["name"], c.start_min)]
            elif op == "max":
                vals = [(f["name"], c.end_max)]
            else:
                src = c.flows if op == "count" else c.bytes if f["inp"] == "Bytes" else c.packets
                vals = [(f["name"] + "_AB", src[0]), (f["name"] + "_BA", src[1])] if f["split"] else [(f["name"], src[0] + src[1])]
            for name, v in vals:
                if v != 0:
                    gm[name] = float(v)
        gm.update(c.keys)
        return gm

    @staticmethod
    def _meta(rec, h, rtype, is_first=None):
        rec["_HashId"] = "%x" % h
        rec["_RecordType"] = rtype
        if is_first is not None:
            rec["_IsFirst"] = is_first
        return rec

    def _get(self, h):                  # store.go:86-107: (connection, its group, active)
        gi = self.group_of.get(h)
        if gi is None:
            return None, None, False
        g = self.groups[gi]
        if h in g["active"].rec:
            return g["active"].rec[h], g, True
        return g["terminating"].rec[h], g, False

    def _walk(self, partials, records, now: int, now_unix_ns: int, mono_now_ns: int, emit):
        """Extract's pass over one call's partials and the store. emit(c, rtype, is_first) renders a conversation record as the
        connection stands at that moment. Returns ({first_idx: newConnection record}, [end records, then heartbeats])."""
        self.now = now
        recs = np.ascontiguousarray(records).view(FLOW_RECORD).reshape(-1)
        parts = np.asarray(partials)
        parts = parts[np.argsort(parts["first_idx"], kind="stable")]
        new_at, to_term, to_back = {}, [], []
        for p in parts:
            h, first_idx, last_idx, fin_idx = int(p["hash_total"]), int(p["first_idx"]), int(p["last_idx"]), int(p["first_fin_idx"])
            same = [int(p["flows"][0]), int(p["bytes"][0]), int(p["packets"][0])]
            other = [int(p["flows"][1]), int(p["bytes"][1]), int(p["packets"][1])]
            c, g, active = self._get(h)
            if c is None:
                if self.max_conns > 0 and len(self.group_of) >= self.max_conns:
                    continue                                          # conntrack.go:88-90: none of its flows is tracked in this call
                r0 = recs[first_idx]
                _, ha, hb = _conn_hash(r0)
                tcp = int(r0["id"]["transport_protocol"]) == 6
                swap = self.swap_ab and tcp and (int(r0["metrics"]["flags"]) & SYN_ACK) == SYN_ACK
                c = _Conn()
                c.hash_a, c.hash_total, c.reported = (hb if swap else ha), h, False
                c.carrier, c.snap_first = _carrier(r0, swap), _snapshot(r0, now_unix_ns, mono_now_ns)
                c.keys = {k: self._field(r0, k, now_unix_ns, mono_now_ns) for k in KEY_FIELDS}
                if swap:
                    c.keys["SrcAddr"], c.keys["DstAddr"] = c.keys["DstAddr"], c.keys["SrcAddr"]
                    c.keys["SrcPort"], c.keys["DstPort"] = c.keys["DstPort"], c.keys["SrcPort"]
                c.first = {f["name"]: self._field(r0, f["inp"], now_unix_ns, mono_now_ns) for f in self.fields if f["op"] == "first"}
                c.expiry = c.next_heartbeat = 0
                gi = next((i for i, gr in enumerate(self.groups) if all(k in c.keys and _text(c.keys[k]) == _text(v) for k, v in gr["selector"].items())),
                          len(self.groups) - 1)
                g, active = self.groups[gi], True
                g["active"].add(h, c)                                  # to the back of both lists, in first_idx order
                self.group_of[h] = gi
                c.next_heartbeat = now + g["hb"]
                # the newConnection record is the connection after its first flow alone (conntrack.go:102-110)
                side = 0 if c.hash_a == ha else 1
                c.flows, c.bytes, c.packets = [0, 0], [0, 0], [0, 0]
                c.flows[side], c.bytes[side], c.packets[side] = 1, int(r0["metrics"]["bytes"]), int(r0["metrics"]["packets"])
                c.start_min = self._field(r0, "TimeFlowStartMs", now_unix_ns, mono_now_ns)
                c.end_max = self._field(r0, "TimeFlowEndMs", now_unix_ns, mono_now_ns)
                c.last = {f["name"]: self._field(r0, f["inp"], now_unix_ns, mono_now_ns) for f in self.fields if f["op"] == "last"}
                c.snap_last = c.snap_first
                if "newConnection" in self.out_types:
                    c.reported = True
                    new_at[first_idx] = emit(c, "newConnection", True)
                c.flows, c.bytes, c.packets = [0, 0], [0, 0], [0, 0]
                c.start_min, c.end_max = int(p["start_ms_min"]), int(p["end_ms_max"])
            else:
                c.start_min, c.end_max = min(c.start_min, int(p["start_ms_min"])), max(c.end_max, int(p["end_ms_max"]))
            ab, ba = (same, other) if int(p["first_hash_a"]) == c.hash_a else (other, same)
            for dst, k in ((c.flows, 0), (c.bytes, 1), (c.packets, 2)):
                dst[0] += ab[k]
                dst[1] += ba[k]
            rl = recs[last_idx]
            c.last = {f["name"]: self._field(rl, f["inp"], now_unix_ns, mono_now_ns) for f in self.fields if f["op"] == "last"}
            c.snap_last = _snapshot(rl, now_unix_ns, mono_now_ns)
            if active:                                                 # a terminating connection stays where it is (store.go:114-117, 143-146)
                if self.detect_end and fin_idx != L.CONN_NO_IDX:
                    to_term.append((fin_idx, h))
                else:
                    to_back.append((last_idx, h))
        for _, h in sorted(to_term):                                   # setConnectionTerminating, in the order of the first FINs
            c, g, _ = self._get(h)
            c.expiry = now + g["term"]
            g["active"].remove(h)
            g["terminating"].add(h, c)
        for _, h in sorted(to_back):                                   # updateConnectionExpiryTime, in the order of the last flows
            c, g, _ = self._get(h)
            c.expiry = now + g["end"]
            del g["active"].expiry[h]
            g["active"].expiry[h] = None
        tail, ended = [], []
        for g in self.groups:                                          # store.go:213-229: per group, terminating before active, front to back
            for lists in (g["terminating"], g["active"]):
                for h in list(lists.expiry):
                    c = lists.rec[h]
                    if not now > c.expiry:
                        break
                    ended.append(c)
                    lists.remove(h)
                    del self.group_of[h]
        if "endConnection" in self.out_types:
            for c in ended:
                first, c.reported = not c.reported, True
                tail.append(emit(c, "endConnection", first))
        if "heartbeat" in self.out_types:
            for g in self.groups:                                      # store.go:231-251
                lists = g["active"]
                for h in list(lists.heartbeat):
                    c = lists.rec[h]
                    if not now > c.next_heartbeat:
                        break
                    c.next_heartbeat = now + g["hb"]
                    del lists.heartbeat[h]
                    lists.heartbeat[h] = None
                    first, c.reported = not c.reported, True
                    tail.append(emit(c, "heartbeat", first))
        return new_at, tail

    def apply(self, partials, records, now: int, now_unix_ns: int, mono_now_ns: int, hash_ids=None, flow_maps=None) -> list:
        """Extract over one call's partials (CONN_PARTIAL, any order) and the records they were folded from. now: the call's
        clock in nanoseconds. With the flowLog type on, hash_ids (the fold's) is needed, and flow_maps[i], when given, is the
        map of flow i to copy into its record; without it a flowLog record is {"_flow": i} beside the two meta fields."""
        new_at, tail = self._walk(partials, records, now, now_unix_ns, mono_now_ns,
                                  lambda c, rtype, is_first: self._meta(self._to_map(c), c.hash_total, rtype, is_first))
        out = []
        if "flowLog" in self.out_types:
            if hash_ids is None:
                raise ValueError("the flowLog record type needs the fold's hash_ids")
            for i in np.nonzero(_tracked(records))[0].tolist():
                if i in new_at:
                    out.append(new_at[i])
                fl = dict(flow_maps[i]) if flow_maps is not None else {"_flow": i}
                out.append(self._meta(fl, int(hash_ids[i]), "flowLog"))
        else:
            out += [new_at[i] for i in sorted(new_at)]
        return out + tail

    def _fold(self, table, records, now_unix_ns: int, mono_now_ns: int, cap: int):
        """(partials, hash_ids or None) of one call; cap doubles while the call has more connections than it."""
        want_ids = "flowLog" in self.out_types
        while True:
            rc, parts, n_conns, ids, _ = table.conn_fold(records, now_unix_ns, mono_now_ns, cap=cap, hash_ids=want_ids)
            if rc == L.OK:
                return parts, ids
            if cap >= L.CONN_MAX_CONNS:
                raise ValueError("more than %d connections in one call" % L.CONN_MAX_CONNS)
            cap = min(max(2 * cap, n_conns), L.CONN_MAX_CONNS)

    def extract(self, table, records, now: int, now_unix_ns: int, mono_now_ns: int, cap: int = 4096, flow_maps=None) -> list:
        """Extract(flowLogs) for the records of one call: the fold on table's device, then apply(). cap doubles while the call
        has more connections than it, up to L.CONN_MAX_CONNS."""
        parts, ids = self._fold(table, records, now_unix_ns, mono_now_ns, cap)
        return self.apply(parts, records, now, now_unix_ns, mono_now_ns, hash_ids=ids, flow_maps=flow_maps)

    # ---- the conversation records as the arrays FlowTable.encode_conn_json takes, and the stage's output as lines
    def conversations(self, partials, records, now: int, now_unix_ns: int, mono_now_ns: int):
        """apply() with the call's conversation records as arrays instead of dicts: (carriers FLOW_RECORD[m], values CONN_VALUES[m],
        order int64[m]), in the order Extract emits them. order[j] is the index of the flow in front of whose record a
        newConnection record goes; it is the number of records for an endConnection or heartbeat record, which follow every
        flow. Flow logs are not part of it: they are the records themselves (FlowTable.encode_flp_json_conn)."""
        from .table import CONN_VALUES
        n = np.ascontiguousarray(records).nbytes // 144

        def row(c, rtype, is_first):
            v = np.zeros((), dtype=CONN_VALUES)
            v["hash_total"], v["record_type"], v["is_first"] = c.hash_total, L.CONN_RECORD_TYPES[rtype], 1 if is_first else 0
            for name, src in (("flows", c.flows), ("bytes", c.bytes), ("packets", c.packets)):
                if max(src) > _M64:
                    raise OverflowError("connection %x: %s above 2^64" % (c.hash_total, name))
                v[name] = src
            v["start_ms_min"], v["end_ms_max"], v["first"], v["last"] = c.start_min, c.end_max, c.snap_first, c.snap_last
            return c.carrier, v

        new_at, tail = self._walk(partials, records, now, now_unix_ns, mono_now_ns, row)
        rows = [(i, new_at[i]) for i in sorted(new_at)] + [(n, r) for r in tail]
        carriers, values = np.zeros(len(rows), dtype=FLOW_RECORD), np.zeros(len(rows), dtype=CONN_VALUES)
        for j, (_, (car, val)) in enumerate(rows):
            carriers[j], values[j] = car, val
        return carriers, values, np.array([i for i, _ in rows], dtype=np.int64)

    def format_deferred(self, table, carrier, values, layout, k8s, net) -> bytes:
        """The line of a conversation the device deferred (an aggregate of magnitude >= 2^53), formatted here. Only the aggregate
        columns need the shortest-float digits, so the device writes the line once more with the aggregates zeroed, which omits
        exactly those columns, and the host puts them back in their places in the sorted order: the layout's key fragment and
        the digits of jsoniter's WriteFloat64 (strconv 'f', precision -1: the shortest digits that round-trip, padded with zeros)."""
        v = np.array(values, dtype=values.dtype).reshape(1)
        agg = {(src, side): _agg_value(v[0], src, side) for src in _AGG_SOURCES for side in (0, 1, 2)}
        for name in _AGG_SOURCES:
            v[name] = 0
        buf, off, deferred = table.encode_conn_json(np.array(carrier, dtype=FLOW_RECORD).reshape(1), v, layout, k8s, net)
        assert not deferred[0] and off[1] == len(buf)
        members = _members(bytes(buf[:-2]))                          # without }\n
        out, at = [], 0
        for k, (name, kind, arg) in enumerate(self._columns()):
            if kind == "agg":
                if agg[arg] != 0:
                    out.append(layout.render(k)[1:] + _float_f(agg[arg]))
            elif kind == "block":                                     # no field name may begin with a block's: its members are contiguous
                while at < len(members) and members[at].startswith(b'"' + name):
                    out.append(members[at])
                    at += 1
            else:
                out.append(members[at])
                at += 1
        assert at == len(members) and k + 1 == layout.n_columns
        return b"{" + b",".join(out) + b"}\n"

    def _columns(self):
        """The columns of a conversation line in the layout's order (byte order; a block sorts as its prefix): [(name, kind, arg)],
        kind "agg" with arg (source, side: 0 both, 1 AB, 2 BA), "block", or "one" for a column that is always one member."""
        cols = [(k.encode(), "one", None) for k in KEY_FIELDS + ("_HashId", "_IsFirst", "_RecordType")]
        cols += [(k, "block", None) for k in (b"DstK8S_", b"DstSubnetLabel", b"K8S_FlowLayer", b"SrcK8S_", b"SrcSubnetLabel")]
        for f in self.fields:
            name = f["name"].encode("latin-1")
            if f["op"] in ("first", "last"):
                cols.append((name, "one", None))
                continue
            src = "flows" if f["op"] == "count" else "start_ms_min" if f["op"] == "min" else "end_ms_max" if f["op"] == "max" else f["inp"].lower()
            cols += [(name + b"_AB", "agg", (src, 1)), (name + b"_BA", "agg", (src, 2))] if f["split"] else [(name, "agg", (src, 0))]
        keys = [k.encode() for k in KEY_FIELDS]
        return sorted(c for k, c in enumerate(cols) if k < len(keys) or c[0] not in keys)      # the keys prevail

    def extract_lines(self, table, records, now: int, now_unix_ns: int, mono_now_ns: int, names, tls_names, k8s, net, agent_ip=None,
                      time_received: int = 0, unknown: bytes = b"unknown", layout=None, cap: int = 4096, present=None, parts=None, rows=None,
                      netev_table=None) -> bytes:
        """Extract for the records of one call as the bytes a direct-FLP pipeline writes behind it: the fold and apply, the flow logs
        through FlowTable.encode_flp_json_conn (when the flowLog type is on), the conversation records through
        FlowTable.encode_conn_json, a deferred one through format_deferred, and the lines in Extract's order: a newConnection
        record in front of its first flow's line, behind the flows the endConnection records, then the heartbeats. names,
        agent_ip, time_received, unknown, present .. netev_table: as encode_flp_json_conn takes them. layout: self.layout(table),
        built for the call when not given."""
        own = layout is None
        layout = self.layout(table) if own else layout
        try:
            folded, ids = self._fold(table, records, now_unix_ns, mono_now_ns, cap)
            carriers, values, order = self.conversations(folded, records, now, now_unix_ns, mono_now_ns)
            buf, off, deferred = table.encode_conn_json(carriers, values, layout, k8s, net)
            buf = buf.tobytes()
            conv = [buf[int(off[j]):int(off[j + 1])] if not deferred[j] else self.format_deferred(table, carriers[j], values[j], layout, k8s, net)
                    for j in range(len(order))]
            if "flowLog" not in self.out_types:
                return b"".join(conv)
            fbuf, foff = table.encode_flp_json_conn(records, tls_names, k8s, net, ids, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown,
                                                    present=present, parts=parts, rows=rows, netev_table=netev_table)
            fbuf, out, at = fbuf.tobytes(), [], 0
            for j, i in enumerate(order.tolist()):                   # the flows' lines up to flow i, then conversation j
                out += [fbuf[int(foff[at]):int(foff[i])], conv[j]]
                at = i
            return b"".join(out) + fbuf[int(foff[at]):]
        finally:
            if own:
                layout.close()


_AGG_SOURCES = ("flows", "bytes", "packets", "start_ms_min", "end_ms_max")


def _agg_value(v, src, side) -> int:
    """An aggregate column's integer: side 0 both (or the time), 1 AB, 2 BA."""
    if src in ("start_ms_min", "end_ms_max"):
        return int(v[src])
    return int(v[src][0]) + int(v[src][1]) if side == 0 else int(v[src][side - 1])


def _float_f(v: int) -> bytes:
    """strconv.FormatFloat(float64(v), 'f', -1, 64): repr() has the shortest digits that round-trip; 'f' pads them with zeros."""
    from decimal import Decimal
    return format(Decimal(repr(float(v))), "f").split(".")[0].encode()


def _members(body: bytes) -> list:
    """The members of one JSON object's text without its closing brace, split at the commas outside strings and arrays."""
    out, start, depth, k = [], 1, 0, 1
    while k < len(body):
        ch = body[k]
        if ch == 0x22:                                                # a string: to its closing quote, over escapes
            k += 1
            while body[k] != 0x22:
                k += 2 if body[k] == 0x5C else 1
        elif ch in (0x5B, 0x7B):
            depth += 1
        elif ch in (0x5D, 0x7D):
            depth -= 1
        elif ch == 0x2C and depth == 0:
            out.append(body[start:k])
            start = k + 1
        k += 1
    return out + [body[start:]]


def _tracked(records):
    """The flows the stage's filter keeps (an IP ethertype and protocol 6, 17 or 132): those with SrcPort and DstPort."""
    recs = np.ascontiguousarray(records).view(FLOW_RECORD).reshape(-1)
    return np.isin(recs["metrics"]["eth_protocol"], (0x0800, 0x86DD)) & np.isin(recs["id"]["transport_protocol"], (6, 17, 132))


def _carrier(r0, swap: bool):
    """The flow record that carries a connection's keys: the addresses and ports of its first flow (swapped by swapAB), the
    protocol and the ethertype."""
    c = np.zeros((), dtype=FLOW_RECORD)
    a, b = ("dst", "src") if swap else ("src", "dst")
    c["id"]["src_ip"], c["id"]["dst_ip"] = r0["id"][a + "_ip"], r0["id"][b + "_ip"]
    c["id"]["src_port"], c["id"]["dst_port"] = r0["id"][a + "_port"], r0["id"][b + "_port"]
    c["id"]["transport_protocol"], c["metrics"]["eth_protocol"] = r0["id"]["transport_protocol"], r0["metrics"]["eth_protocol"]
    return c


def _snapshot(rec, now_unix_ns: int, mono_now_ns: int):
    """nfagg_conn_snapshot of one flow: what FIRST_LAST_FIELDS can copy from it."""
    from .table import CONN_SNAPSHOT
    k, m = rec["id"], rec["metrics"]
    s = np.zeros((), dtype=CONN_SNAPSHOT)
    for name in ("src_ip", "dst_ip", "src_port", "dst_port"):
        s[name] = k[name]
    s["proto"], s["eth_protocol"], s["dscp"], s["src_mac"], s["dst_mac"] = k["transport_protocol"], m["eth_protocol"], m["dscp"], m["src_mac"], m["dst_mac"]
    dirs = ConnTrack._field(rec, "IfDirections", now_unix_ns, mono_now_ns)
    s["n_dirs"] = len(dirs)
    s["dirs"][:len(dirs)] = dirs
    s["start_ms"] = unix_milli(now_unix_ns, mono_now_ns, int(m["start_mono_time_ts"]))
    s["end_ms"] = unix_milli(now_unix_ns, mono_now_ns, int(m["end_mono_time_ts"]))
    return s


def _conn_hash(rec):
    from .table import conn_hash
    return conn_hash(rec.tobytes())
