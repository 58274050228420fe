"""Independent restatement of flowlogs-pipeline's `extract conntrack`, one flow at a time, for the tests (no import of the
product). Its input is the maps of flp_json_ref.record_to_map (keys and strings are bytes); paths below are under
vendor/github.com/netobserv/flowlogs-pipeline/pkg:

  api/conntrack.go:105-229                    Validate
  config/generic_map.go:44-69                 IsDuplicate, IsValidProtocol, IsTransportProtocol
  pipeline/extract/conntrack/conntrack.go     59-64 filterFlowLog, 66-142 Extract, 144-180 the end and heartbeat records,
                                              182-225 updateConnection, containsTCPFlag, getFlowLogDirection
  pipeline/extract/conntrack/hash.go          41-73 computeHash, 75-93 computeHashFields, 95-110 uint64ToBytes, toBytes
  pipeline/extract/conntrack/aggregator.go    58-93 newAggregator, 95-142, 144-199 the six updates
  pipeline/extract/conntrack/conn.go          101-114 toGenericMap, 120-124 markReported, 127-178 isMatchSelector, 197-226 the builder
  pipeline/extract/conntrack/store.go         58-255 the store: two ordered lists per group and phase
  pipeline/extract/conntrack/tcpflags.go      FIN 0x01, SYN_ACK 0x100
  Go hash/fnv New64a; encoding/gob's message for a string, a uint16 and a uint8

The gob bytes are written from encoding/gob's documentation, not checked against a Go run: _HashId is pinned to THIS file.
One difference from the reference, stated: extract() takes one `now` (nanoseconds) per call where the reference reads its
clock several times per Extract."""
import re

M64 = (1 << 64) - 1
FNV_OFFSET, FNV_PRIME = 0xcbf29ce484222325, 0x100000001b3
FIN, SYN_ACK = 0x01, 0x100
MAX_FLOAT64 = 1.7976931348623157e308
RECORD_TYPES = ("newConnection", "endConnection", "heartbeat", "flowLog")
_UNITS = {"ns": 1, "us": 10**3, "µs": 10**3, "μs": 10**3, "ms": 10**6, "s": 10**9, "m": 60 * 10**9, "h": 3600 * 10**9}


def parse_duration(v) -> int:
    """time.ParseDuration, as far as configurations use it: "1m30s", "500ms", "0"; an int is nanoseconds."""
    if isinstance(v, (int, float)):
        return int(v)
    if v in ("0", "", None):
        return 0
    parts = re.findall(r"([0-9]*\.?[0-9]+)(ns|us|µs|μs|ms|s|m|h)", v)
    if not parts or "".join(a + b for a, b in parts) != v.lstrip("+"):
        raise ValueError("invalid duration %r" % (v,))
    return sum(int(round(float(a) * _UNITS[u])) for a, u in parts)


# ---- hash.go

def fnv64a(data: bytes, h: int = FNV_OFFSET) -> int:
    for b in data:
        h = ((h ^ b) * FNV_PRIME) & M64
    return h


def gob_uint(v: int) -> bytes:
    """encoding/gob's unsigned integer: below 128 one byte; else the negated byte count, then the minimal big-endian bytes."""
    if v < 128:
        return bytes([v])
    raw = v.to_bytes((v.bit_length() + 7) // 8, "big")
    return bytes([256 - len(raw)]) + raw


def to_bytes(value) -> bytes:
    """hash.go:101-110 toBytes: a fresh gob.Encoder's message for one value, [byte count][type id, zigzag][0x00][value].
    bytes: a Go string (type id 6 -> 0x0c); int: a uint16 or uint8 (type id 3 -> 0x06)."""
    if isinstance(value, (bytes, bytearray)):
        body = b"\x0c\x00" + gob_uint(len(value)) + bytes(value)
    else:
        body = b"\x06\x00" + gob_uint(int(value))
    return gob_uint(len(body)) + body


def compute_hash(flow: dict, key_definition: dict):
    """hash.go:41-73: (hashA, hashB, hashTotal). A field the flow lacks is skipped (hash.go:78-85)."""
    group_hash = {}
    for fg in key_definition.get("fieldGroups", []):
        h = FNV_OFFSET
        for f in fg.get("fields", []):
            k = f.encode()
            if k in flow:
                h = fnv64a(to_bytes(flow[k]), h)
        group_hash[fg["name"]] = h
    hd = key_definition.get("hash", {})
    h = FNV_OFFSET
    for ref in hd.get("fieldGroupRefs", []):
        h = fnv64a(group_hash.get(ref, 0).to_bytes(8, "big"), h)
    a = b = 0
    if hd.get("fieldGroupARef", ""):
        a, b = group_hash.get(hd["fieldGroupARef"], 0), group_hash.get(hd["fieldGroupBRef"], 0)
        lo, hi = (a, b) if a < b else (b, a)
        h = fnv64a(hi.to_bytes(8, "big"), fnv64a(lo.to_bytes(8, "big"), h))
    return a, b, h


# ---- api/conntrack.go:105-229

def validate(cfg: dict) -> None:
    kd = cfg.get("keyDefinition", {})
    hd = kd.get("hash", {})
    a_ref, b_ref = hd.get("fieldGroupARef", ""), hd.get("fieldGroupBRef", "")
    if (a_ref == "") != (b_ref == ""):
        raise ValueError("only one of 'fieldGroupARef' and 'fieldGroupBRef' is set. They should both be set or both unset")
    bidi = a_ref != ""
    for of in cfg.get("outputFields", []):
        if of.get("splitAB", False) and not bidi:
            raise ValueError("output field %r has splitAB=true although bidirection is not enabled (fieldGroupARef is empty)" % of.get("name", ""))
        op, split = of.get("operation", ""), of.get("splitAB", False)
        if op not in ("sum", "count", "min", "max", "first", "last") or (op in ("first", "last") and split):
            raise ValueError("unknown operation %r in output field %r" % (op, of.get("name", "")))
    names = set()
    for of in cfg.get("outputFields", []):
        for name in ([of.get("name", "") + "_AB", of.get("name", "") + "_BA"] if of.get("splitAB", False) else [of.get("name", "")]):
            if name in names:
                raise ValueError("duplicate outputField %r" % name)
            names.add(name)
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
        for k in g.get("selector", {}) or {}:
            if k not in keys:
                raise ValueError("selector key %r in scheduling group %d is not defined in the keys" % (k, i))
    n_default = 0
    for i, g in enumerate(sched):
        if not (g.get("selector", {}) or {}):
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
    fa, fb = ab_fields(cfg)
    if len(fa) != len(fb):
        raise ValueError("mismatch between the field count of fieldGroupARef %d and fieldGroupBRef %d" % (len(fa), len(fb)))


def ab_fields(cfg: dict):
    kd = cfg.get("keyDefinition", {})
    hd = kd.get("hash", {})
    fa, fb = [], []
    for fg in kd.get("fieldGroups", []):
        if fg.get("name", "") == hd.get("fieldGroupARef", ""):
            fa = fg.get("fields", [])
        if fg.get("name", "") == hd.get("fieldGroupBRef", ""):
            fb = fg.get("fields", [])
    return fa, fb


def _go_v(v) -> bytes:
    """fmt.Sprintf("%v") / ConvertToString of a selector value or a key value, as bytes."""
    if isinstance(v, (bytes, bytearray)):
        return bytes(v)
    if isinstance(v, bool):
        return b"true" if v else b"false"
    if isinstance(v, float) and v == int(v):
        v = int(v)
    return str(v).encode()


class _Conn:
    def __init__(self):
        self.hash = (0, 0, 0)             # hashA, hashB, hashTotal
        self.keys = {}
        self.agg = {}                     # insertion ordered, like nothing in Go: toGenericMap's result is a map anyway
        self.expiry = 0
        self.next_heartbeat = 0
        self.reported = False

    def to_map(self) -> dict:             # conn.go:101-114
        gm = {k: v for k, v in self.agg.items() if v is not None and not (isinstance(v, float) and v == 0)}
        gm.update(self.keys)
        return gm

    def mark_reported(self) -> bool:
        first = not self.reported
        self.reported = True
        return first

    def matches(self, selector: dict) -> bool:      # conn.go:127-178: a uint8 / uint16 / string key compares as text
        for k, v in selector.items():
            kb = k.encode()
            if kb not in self.keys or _go_v(self.keys[kb]) != _go_v(v):
                return False
        return True


class _Mom:
    """utils.MultiOrderedMap with the two orders the store uses: records by key, one ordered list per order."""
    def __init__(self):
        self.rec, self.order = {}, {"expiry": {}, "heartbeat": {}}

    def add(self, key, rec):
        self.rec[key] = rec
        for o in self.order.values():
            o[key] = None

    def remove(self, key):
        del self.rec[key]
        for o in self.order.values():
            del o[key]

    def move_to_back(self, key, order):
        del self.order[order][key]
        self.order[order][key] = None


class ConnTrack:
    def __init__(self, config: dict):
        validate(config)
        self.cfg = config
        self.kd = config.get("keyDefinition", {})
        self.fields_a, self.fields_b = ab_fields(config)
        self.bidi = self.kd.get("hash", {}).get("fieldGroupARef", "") != ""
        tf = config.get("tcpFlags", {})
        self.flags_field = tf.get("fieldName", "").encode()
        self.detect_end, self.swap_ab = tf.get("detectEndConnection", False), tf.get("swapAB", False)
        self.max_conns = config.get("maxConnectionsTracked", 0)
        self.out_types = set(config.get("outputRecordTypes", []))
        self.aggs = []
        for of in config.get("outputFields", []):                      # aggregator.go:58-93
            if not of.get("name", ""):
                raise ValueError("empty name %r" % (of,))
            op = of["operation"]
            init = {"sum": 0.0, "count": 0.0, "min": MAX_FLOAT64, "max": -MAX_FLOAT64, "first": None, "last": None}[op]
            self.aggs.append(dict(op=op, out=of["name"].encode(), inp=(of.get("input", "") or of["name"]).encode(), split=of.get("splitAB", False),
                                  init=init, report_missing=of.get("reportMissing", False)))
        self.groups = [dict(selector=g.get("selector", {}) or {}, end=parse_duration(g.get("endConnectionTimeout", 0)),
                            term=parse_duration(g.get("terminatingTimeout", 0)), hb=parse_duration(g.get("heartbeatInterval", 0)),
                            active=_Mom(), terminating=_Mom()) for g in config.get("scheduling", [])]
        self.group_of = {}                # hashID2groupIdx
        self.now = 0

    # ---- store.go
    def _get(self, h):                    # (conn, exists, active)
        if h not in self.group_of:
            return None, False, False
        g = self.groups[self.group_of[h]]
        if h in g["active"].rec:
            return g["active"].rec[h], True, True
        if h in g["terminating"].rec:
            return g["terminating"].rec[h], True, False
        return None, False, False

    def _add(self, h, conn):
        gi = next((i for i, g in enumerate(self.groups) if conn.matches(g["selector"])), len(self.groups) - 1)
        self.groups[gi]["active"].add(h, conn)
        self.group_of[h] = gi

    def _set_terminating(self, h):
        conn, _, active = self._get(h)
        if not active:
            return
        g = self.groups[self.group_of[h]]
        conn.expiry = self.now + g["term"]
        g["active"].remove(h)
        g["terminating"].add(h, conn)

    def _update_expiry(self, h):
        conn, _, active = self._get(h)
        if not active:
            return
        g = self.groups[self.group_of[h]]
        conn.expiry = self.now + g["end"]
        g["active"].move_to_back(h, "expiry")

    def _update_heartbeat(self, h):
        conn, _, active = self._get(h)
        if not active:
            return
        g = self.groups[self.group_of[h]]
        conn.next_heartbeat = self.now + g["hb"]
        g["active"].move_to_back(h, "heartbeat")

    def _pop_end(self):
        out = []
        for g in self.groups:
            for mom in (g["terminating"], g["active"]):                # terminating first (store.go:217-226)
                for h in list(mom.order["expiry"]):
                    conn = mom.rec[h]
                    if not self.now > conn.expiry:                     # now.After(expiry)
                        break
                    out.append(conn)
                    mom.remove(h)
                    del self.group_of[h]
        return out

    def _heartbeats(self):
        out = []
        for g in self.groups:
            mom = g["active"]
            for h in list(mom.order["heartbeat"]):                     # IterateFrontToBack reads next before the callback moves the element
                conn = mom.rec[h]
                if not self.now > conn.next_heartbeat:
                    break
                out.append(conn)
                self._update_heartbeat(h)
        return out

    # ---- aggregator.go
    def _out_field(self, a, d):
        return a["out"] + ((b"_AB" if d == "AB" else b"_BA") if a["split"] else b"")

    def _value(self, a, flow):            # (float, ok)
        if a["inp"] not in flow:
            return 0.0, not a["report_missing"]
        return float(flow[a["inp"]]), True

    def _update(self, conn, flow, h3, is_new):
        d = None
        if self.bidi:
            d = "AB" if conn.hash[0] == h3[0] else "BA"
        for a in self.aggs:
            op = a["op"]
            if op in ("first", "last"):
                v = flow.get(a["inp"])
                if (op == "first" and is_new) or (op == "last" and v is not None):
                    conn.agg[a["out"]] = v
                continue
            f = self._out_field(a, d)
            if op == "count":
                conn.agg[f] += 1.0
                continue
            v, ok = self._value(a, flow)
            if not ok:
                continue
            conn.agg[f] = conn.agg[f] + v if op == "sum" else min(conn.agg[f], v) if op == "min" else max(conn.agg[f], v)
        if self.detect_end and self._has_flag(flow, FIN):
            self._set_terminating(h3[2])
        else:
            self._update_expiry(h3[2])

    def _has_flag(self, flow, q):
        return self.flags_field in flow and (int(flow[self.flags_field]) & q) == q

    @staticmethod
    def _meta(rec, h, rtype, is_first=None):
        rec[b"_HashId"] = b"%x" % h
        rec[b"_RecordType"] = rtype.encode()
        if is_first is not None:
            rec[b"_IsFirst"] = is_first
        return rec

    # ---- conntrack.go:66-142
    def extract(self, flows, now: int):
        self.now = now
        out = []
        for fl in flows:
            if b"Proto" not in fl or fl[b"Proto"] not in (6, 17, 132):
                continue
            h3 = compute_hash(fl, self.kd)
            conn, exists, _ = self._get(h3[2])
            if not exists:
                if self.max_conns > 0 and len(self.group_of) >= self.max_conns:
                    pass                                               # too many connections: the flow is not tracked
                else:
                    conn = _Conn()
                    swap = self.swap_ab and self._has_flag(fl, SYN_ACK)
                    conn.hash = (h3[1], h3[0], h3[2]) if swap else h3
                    for fg in self.kd.get("fieldGroups", []):
                        for f in fg.get("fields", []):
                            conn.keys[f.encode()] = fl.get(f.encode())
                    if swap:
                        for fa, fb in zip(self.fields_a, self.fields_b):
                            conn.keys[fa.encode()], conn.keys[fb.encode()] = fl.get(fb.encode()), fl.get(fa.encode())
                    for a in self.aggs:
                        for f in ([a["out"] + b"_AB", a["out"] + b"_BA"] if a["split"] else [a["out"]]):
                            conn.agg[f] = a["init"]
                    self._add(h3[2], conn)
                    self._update_heartbeat(h3[2])
                    self._update(conn, fl, h3, True)
                    if "newConnection" in self.out_types:
                        out.append(self._meta(conn.to_map(), h3[2], "newConnection", conn.mark_reported()))
            else:
                self._update(conn, fl, h3, False)
            if "flowLog" in self.out_types:
                out.append(self._meta(dict(fl), h3[2], "flowLog"))
        ended = self._pop_end()
        if "endConnection" in self.out_types:
            out += [self._meta(c.to_map(), c.hash[2], "endConnection", c.mark_reported()) for c in ended]
        if "heartbeat" in self.out_types:
            out += [self._meta(c.to_map(), c.hash[2], "heartbeat", c.mark_reported()) for c in self._heartbeats()]
        return out


def fold(flows, key_definition):
    """What nfagg_conn_fold computes, restated per flow: (partials, hash_ids, n_discarded). A partial is a dict of
    nfagg_conn_partial's fields; partials come in first_idx order."""
    conns, ids, discarded = {}, [], 0
    for i, fl in enumerate(flows):
        if b"Proto" not in fl or fl[b"Proto"] not in (6, 17, 132):
            ids.append(0)
            discarded += 1
            continue
        a, _, h = compute_hash(fl, key_definition)
        ids.append(h)
        p = conns.get(h)
        if p is None:
            p = conns[h] = dict(hash_total=h, first_hash_a=a, first_idx=i, last_idx=i, first_fin_idx=0xFFFFFFFF, flags_or=0, flows=[0, 0], bytes=[0, 0],
                                packets=[0, 0], start_ms_min=fl[b"TimeFlowStartMs"], end_ms_max=fl[b"TimeFlowEndMs"])
        side = 0 if a == p["first_hash_a"] else 1
        p["last_idx"] = i
        p["flows"][side] += 1
        p["bytes"][side] = (p["bytes"][side] + fl.get(b"Bytes", 0)) & M64
        p["packets"][side] = (p["packets"][side] + fl.get(b"Packets", 0)) & M64
        p["start_ms_min"], p["end_ms_max"] = min(p["start_ms_min"], fl[b"TimeFlowStartMs"]), max(p["end_ms_max"], fl[b"TimeFlowEndMs"])
        if b"Flags" in fl:
            p["flags_or"] |= fl[b"Flags"]
            if fl[b"Flags"] & FIN and p["first_fin_idx"] == 0xFFFFFFFF:
                p["first_fin_idx"] = i
    return list(conns.values()), ids, discarded
