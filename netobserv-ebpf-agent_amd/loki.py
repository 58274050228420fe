"""flowlogs-pipeline's `write loki` stage over the device path (include/nfagg.h, "write loki on the device").

WriteLoki mirrors NewWriteLoki (pkg/pipeline/write/write_loki.go:310-375): the defaults of api/write_loki.go:62-87, the label
names sanitized by keyReplacer and checked by LegacyValidation, the ignore list. It compiles the stage into the two key masks
of nfagg_loki_spec; what the masks cannot say raises ValueError, and such a stage stays on the host path. LokiTable is the
stage over a Kubernetes and a net table (nfagg_loki_table_create); FlowTable.loki_plan / loki_write are the two calls;
LokiWriter turns one eviction into the list of PushRequest bodies (snappy and the send stay with the caller).

labelset_string is LabelSet.String() (prometheus/common/model/labelset_string.go:23-43) for ASCII values, strconv.AppendQuote's
escapes included. A value with a rune outside ASCII raises: strconv.IsPrint's table is not restated here, and the C ABI takes
the rendered text from the caller for the same reason."""
import ctypes as C
import re

import numpy as np

from . import _lib as L
from .metrics import K8S_SUFFIXES, KEY_DIMS, _field_present, _b
from .records import INTF_NAME
from .table import K8S_FIELDS, NfaggError, _CallerTable, flp_options

LOKI_STREAM = np.dtype([("src_class", "<u4"), ("dst_class", "<u4"), ("src_label", "<u2"), ("dst_label", "<u2"), ("direction", "u1"),
                        ("layer", "u1"), ("record_type", "u1"), ("pad_", "u1"), ("first_flow", "<u4")])          # nfagg_loki_stream
LOKI_GROUP = np.dtype([("batch", "<u4"), ("stream", "<u4"), ("n_entries", "<u4"), ("pad_", "<u4"), ("entry_bytes", "<u8")])   # nfagg_loki_group
assert LOKI_STREAM.itemsize == 20 and LOKI_GROUP.itemsize == 24

# the keys a mask can name: the hooks of the line policies
LOKI_KEYS = {k: v for k, v in KEY_DIMS.items() if k != "Proto"}
LOKI_KEYS.update(_RecordType=L.LOKI_KEY_RECORD_TYPE, _HashId=L.LOKI_KEY_HASH_ID)
TIMESTAMP_SOURCES = {"TimeFlowEndMs": L.LOKI_TS_TIME_FLOW_END_MS, "TimeFlowStartMs": L.LOKI_TS_TIME_FLOW_START_MS}
_DURATION_UNITS = {"ns": 1, "us": 1000, "µs": 1000, "μs": 1000, "ms": 10 ** 6, "s": 10 ** 9, "m": 60 * 10 ** 9, "h": 3600 * 10 ** 9}
_LEGACY_NAME = re.compile(r"^[a-zA-Z_][a-zA-Z0-9_]*$")          # model.LegacyValidation.IsValidLabelName
MIN_SECONDS, MAX_SECONDS = -62135596800, 253402300800            # timestamp.go:31-36: [year 1, year 10000)


def parse_duration(text: str) -> int:
    """time.ParseDuration for the forms a configuration uses: [-+]?([0-9]*(\\.[0-9]*)?[a-z]+)+, in nanoseconds."""
    m = re.fullmatch(r"([-+]?)((?:\d*\.?\d*(?:ns|us|µs|μs|ms|s|m|h))+)", text)
    if text in ("0", "+0", "-0"):
        return 0
    if not m:
        raise ValueError("time: invalid duration %r" % text)
    total = 0
    for num, unit in re.findall(r"(\d*\.?\d*)(ns|us|µs|μs|ms|s|m|h)", m.group(2)):
        if num in ("", "."):
            raise ValueError("time: invalid duration %r" % text)
        whole, _, frac = num.partition(".")
        total += int(whole or "0") * _DURATION_UNITS[unit]
        if frac:
            total += int(frac) * _DURATION_UNITS[unit] // 10 ** len(frac)
    return -total if m.group(1) == "-" else total


def sanitize(key: str) -> str:
    """keyReplacer (write_loki.go:42)."""
    return key.replace("/", "_").replace(".", "_").replace("-", "_")


def go_quote(value) -> bytes:
    """strconv.AppendQuote of an ASCII string."""
    out = bytearray(b'"')
    short = {0x07: b"\\a", 0x08: b"\\b", 0x0c: b"\\f", 0x0a: b"\\n", 0x0d: b"\\r", 0x09: b"\\t", 0x0b: b"\\v", 0x22: b'\\"', 0x5c: b"\\\\"}
    for b in _b(value):
        if b >= 0x80:
            raise ValueError("labelset_string serves ASCII values: strconv.IsPrint's table is not restated")
        out += short[b] if b in short else b"\\x%02x" % b if b < 0x20 or b == 0x7f else bytes([b])
    return bytes(out + b'"')


def labelset_string(labels: dict) -> bytes:
    """LabelSet.String(): {a="..", b=".."}, names sorted, values through strconv.AppendQuote."""
    return b"{" + b", ".join(_b(name) + b"=" + go_quote(labels[name]) for name in sorted(labels, key=_b)) + b"}"


def extract_timestamp(value, scale: float, now_unix_ns: int):
    """extractTimestamp (write_loki.go:253-277) as (seconds, nanos) of the time.Time, or None when the float64 product leaves
    int64. value None: the key is not in the line."""
    if value is None or float(value) == 0.0:
        tn = int(now_unix_ns)
    else:
        prod = float(value) * float(scale)
        if not (-9223372036854775808.0 <= prod < 9223372036854775808.0):
            return None
        tn = int(prod)
    sec, nsec = abs(tn) // 10 ** 9, abs(tn) % 10 ** 9                 # Go's / and % truncate
    if tn < 0:
        sec, nsec = -sec, -nsec
    if nsec < 0:                                                      # time.Unix normalizes
        sec, nsec = sec - 1, nsec + 10 ** 9
    return sec, nsec


class WriteLoki:
    """The stage's configuration, compiled. config: the api.WriteLoki keys as the YAML has them (url, batchSize, labels,
    staticLabels, ignoreList, timestampLabel, timestampScale, format, ...). ValueError for what the device path does not serve: a
    label or an ignored key outside LOKI_KEYS, _HashId as a label, a format other than json, a timestamp label other than
    TimeFlowEndMs, TimeFlowStartMs, TimeReceived."""

    def __init__(self, config: dict = None):
        c = dict(config or {})
        self.batch_size = int(c.get("batchSize") or 100 * 1024)                      # SetDefaults
        self.batch_wait = c.get("batchWait") or "1s"
        self.timeout = c.get("timeout") or "10s"
        self.min_backoff, self.max_backoff = c.get("minBackoff") or "1s", c.get("maxBackoff") or "1s"
        self.max_retries = int(c.get("maxRetries") or 10)
        self.timestamp_label = c.get("timestampLabel") or "TimeReceived"
        self.timestamp_scale_text = c.get("timestampScale") or "1s"
        self.format = c.get("format") or "json"
        self.client_protocol = c.get("clientProtocol") or "http"
        self.url, self.tenant_id = c.get("url", ""), c.get("tenantID", "")
        self.static_labels = {str(k): _b(v) for k, v in (c.get("staticLabels") or {}).items()}
        if self.batch_size <= 0 or self.batch_size > 2 ** 31 - 1:
            raise ValueError("invalid batchSize: %d" % self.batch_size)
        if self.client_protocol not in ("http", "grpc"):
            raise ValueError("invalid clientProtocol: %s" % self.client_protocol)
        if self.format != "json":
            raise ValueError("format %r stays on the host path: the device writes json lines" % self.format)
        self.timestamp_scale = float(parse_duration(self.timestamp_scale_text))      # float64(time.Duration)
        if self.timestamp_scale <= 0:
            raise ValueError("timestampScale must be a Duration > 0")
        self.ignore_list = list(c.get("ignoreList") or [])
        self.sane_labels = {}                                                        # key -> sanitized name; an invalid name is dropped
        for key in c.get("labels") or []:
            name = sanitize(key)
            if _LEGACY_NAME.match(name):
                self.sane_labels[key] = name
        for key in list(self.sane_labels) + self.ignore_list:
            if key not in LOKI_KEYS:
                raise ValueError("key %r as a label or ignored stays on the host path: the device serves %s" % (key, sorted(LOKI_KEYS)))
        self.ignore_keys = 0
        for key in self.ignore_list:
            self.ignore_keys |= LOKI_KEYS[key]
        self.label_keys = 0
        for key in self.sane_labels:
            if key not in self.ignore_list:
                self.label_keys |= LOKI_KEYS[key]
        if self.label_keys & L.LOKI_KEY_HASH_ID:
            raise ValueError("_HashId as a label stays on the host path: a stream per conversation")
        if self.timestamp_label in TIMESTAMP_SOURCES:
            self.timestamp_source = TIMESTAMP_SOURCES[self.timestamp_label]
        elif self.timestamp_label == "TimeReceived":
            self.timestamp_source = L.LOKI_TS_NOW                                    # one value per call: timestamp_of_call works it out
        else:
            raise ValueError("timestampLabel %r stays on the host path" % self.timestamp_label)

    def spec(self) -> "L.LokiSpec":
        return L.LokiSpec(C.sizeof(L.LokiSpec), self.label_keys, self.ignore_keys, self.timestamp_source, self.timestamp_scale, self.batch_size, 0)

    def now_of_call(self, now_unix_ns: int, time_received: int):
        """What a call passes as timeNow(): with timestampLabel TimeReceived (one value per call, a key no mask can take out of the
        line) the stage's timestamp itself. None: the product leaves int64, every flow is the caller's."""
        if self.timestamp_label != "TimeReceived":
            return int(now_unix_ns)
        t = extract_timestamp(time_received, self.timestamp_scale, now_unix_ns)
        return None if t is None else t[0] * 10 ** 9 + t[1]

    def stream_labels(self, stream, k8s_entries, net_labels, class_row) -> dict:
        """The LabelSet of one stream of a plan: static labels, then the label keys' values under their sanitized names.
        class_row(side, cls) -> the Kubernetes entry whose label fields are the class's."""
        labels = dict(self.static_labels)
        for side, prefix, cls in ((0, "SrcK8S_", int(stream["src_class"])), (1, "DstK8S_", int(stream["dst_class"]))):
            if not cls:
                continue
            info = k8s_entries[class_row(side, cls)][1]
            for f in range(9):
                key = prefix + K8S_SUFFIXES[f]
                if self.label_keys & LOKI_KEYS[key] and _field_present(info, f):
                    value = _b(info.get(K8S_FIELDS[f]) or b"")
                    if _utf8_valid(value):
                        labels[self.sane_labels[key]] = value
        for key, field in (("SrcSubnetLabel", "src_label"), ("DstSubnetLabel", "dst_label")):
            if self.label_keys & LOKI_KEYS[key] and int(stream[field]) != L.NET_NO_LABEL:
                labels[self.sane_labels[key]] = _b(net_labels[int(stream[field])])
        if self.label_keys & L.DIM_FLOW_DIRECTION and int(stream["direction"]) != L.NET_NO_DIRECTION:
            labels[self.sane_labels["FlowDirection"]] = b"%d" % int(stream["direction"])
        if self.label_keys & L.DIM_FLOW_LAYER and int(stream["layer"]):
            labels[self.sane_labels["K8S_FlowLayer"]] = b"app" if int(stream["layer"]) == 2 else b"infra"
        if self.label_keys & L.LOKI_KEY_RECORD_TYPE and int(stream["record_type"]):
            labels[self.sane_labels["_RecordType"]] = b"flowLog"
        return labels


def _utf8_valid(value: bytes) -> bool:
    try:
        value.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


class LokiTable(_CallerTable):
    """nfagg_loki_table_create: a WriteLoki over a K8sTable and a NetTable. With a FlowTable the table lives on its device and
    serves loki_plan; with table=None it is built and checked on the host only (the two tables as well)."""

    def __init__(self, writer: WriteLoki, k8s, net, table=None, spec=None):
        s = spec if spec is not None else writer.spec()
        self._create(table, L.lib.nfagg_loki_table_destroy, lambda h, out: L.lib.nfagg_loki_table_create(h, k8s._t, net._t, C.byref(s), out))
        self.writer, self.k8s, self.net = writer, k8s, net

    def n_classes(self, side: int) -> int:
        return L.lib.nfagg_loki_n_classes(self._t, side)

    def class_row(self, side: int, cls: int) -> int:
        row = C.c_uint32(0)
        rc = L.lib.nfagg_loki_class_row(self._t, side, cls, C.byref(row))
        if rc != L.OK:
            raise NfaggError(rc, (L.lib.nfagg_last_error(None) or b"").decode())
        return row.value

    def render(self, side: int, row: int) -> bytes:
        buf = np.zeros(L.K8S_MAX_RENDERED, dtype=np.uint8)
        n = C.c_size_t(0)
        rc = L.lib.nfagg_loki_render(self._t, side, row, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n))
        if rc != L.OK:
            raise NfaggError(rc, (L.lib.nfagg_last_error(None) or b"").decode())
        return buf[:n.value].tobytes()

    def labels_of(self, streams) -> list:
        """Every stream's LabelSet.String()."""
        return [labelset_string(self.writer.stream_labels(s, self.k8s.entries, self.net.labels, self.class_row)) for s in streams]


def loki_plan(table, records, tls_names, k8s, net, loki: LokiTable, now_unix_ns: int, mono_now_ns: int, names, agent_ip=None, time_received: int = 0,
              unknown: bytes = b"unknown", hash_ids=None, loki_now_ns: int = None, stream_cap: int = None, group_cap: int = None, present=None, parts=None,
              rows=None, netev_table=None):
    """nfagg_loki_plan. present / parts: the feature parts of full flow contents (present None: the plain line); rows and
    netev_table: their resolved network events, as encode_flp_json_conn takes them. Returns (rc, streams, groups, deferred, counts): LOKI_STREAM / LOKI_GROUP arrays, a byte per flow, the
    LokiCounts. The caps grow until the plan fits unless given (then rc may be L.TRUNCATED, with empty arrays)."""
    r = np.ascontiguousarray(records)
    n = r.nbytes // 144
    o, keep = flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown)
    ids = np.ascontiguousarray(hash_ids, dtype=np.uint64) if hash_ids is not None else None
    assert ids is None or ids.size == n
    deferred = np.zeros(n, dtype=np.uint8)
    counts = L.LokiCounts()
    feat = keep_f = None
    if present is not None:
        feat, keep_f = table._pb_features(n, present, table._content_parts(parts))
    rw = np.ascontiguousarray(rows, dtype=np.uint16).reshape(n, 4) if rows is not None else None
    f_args = (C.byref(feat) if feat is not None else None, rw.ctypes.data_as(C.c_void_p) if rw is not None else None,
              netev_table._t if netev_table is not None else None)
    fixed = stream_cap is not None or group_cap is not None
    sc = min(int(stream_cap if stream_cap is not None else 64), L.LOKI_MAX_STREAMS)
    gc = int(group_cap if group_cap is not None else 256)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None  # noqa: E731
    while True:
        streams, groups = np.zeros(sc, dtype=LOKI_STREAM), np.zeros(gc, dtype=LOKI_GROUP)
        rc = L.lib.nfagg_loki_plan(table._h, ptr(r), n, *f_args, tls_names._t, k8s._t, net._t, ptr(ids) if ids is not None else None, C.byref(o),
                                   loki._t, int(loki_now_ns if loki_now_ns is not None else now_unix_ns), ptr(streams), sc, ptr(groups), gc, ptr(deferred),
                                   C.byref(counts))
        table._check(rc, ok=(L.OK, L.TRUNCATED))
        if rc == L.OK or fixed:
            break
        sc, gc = min(max(sc, counts.n_streams), L.LOKI_MAX_STREAMS), max(gc, counts.n_groups)
    k = rc == L.OK
    return rc, streams[:counts.n_streams if k else 0], groups[:counts.n_groups if k else 0], deferred, counts


def loki_write(table, label_texts, n_batches: int, out_cap: int = None):
    """nfagg_loki_write over the handle's plan. label_texts: every stream's LabelSet.String(). Returns (rc, buf, batch_offsets,
    batch_entries); the buffer grows until the bodies fit unless out_cap is given (then rc may be L.TRUNCATED and buf holds
    nothing, batch_offsets[-1] what is needed)."""
    blob = b"".join(label_texts)
    off = np.zeros(len(label_texts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(t) for t in label_texts], dtype=np.uint64)
    boffs, bents = np.zeros(n_batches + 1, dtype=np.uint64), np.zeros(max(n_batches, 1), dtype=np.uint32)
    need = C.c_size_t(0)
    cap = int(out_cap) if out_cap is not None else 0
    while True:
        buf = np.zeros(max(cap, 16), dtype=np.uint8)
        rc = L.lib.nfagg_loki_write(table._h, blob, off.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p) if cap else None, cap,
                                    boffs.ctypes.data_as(C.c_void_p), bents.ctypes.data_as(C.c_void_p), C.byref(need))
        table._check(rc, ok=(L.OK, L.TRUNCATED))
        if rc == L.OK or out_cap is not None:
            break
        cap = need.value
    return rc, buf[:need.value if rc == L.OK else 0], boffs, bents[:n_batches]


class LokiWriter:
    """One eviction through the stage: ExportEvicted returns (bodies, deferred). bodies: the PushRequest bodies in batch order,
    what the Go shim hands to snappy.Encode; deferred: the indexes of the flows the caller formats itself (a timestamp the
    reference would lose the batch over). An `extract conntrack` stage with the flowLog type in front: hand ExportEvicted the
    hash_ids of that stage's fold (ConnTrack's), or set conntrack=True and the writer folds the call itself — a pipeline that has
    a ConnTrack as well would then fold twice, so pass its ids. Untracked flows get no entry. send(body), when given, is called
    per body."""

    def __init__(self, table, writer: WriteLoki, tls_names, k8s, net, names=None, agent_ip=None, unknown: bytes = b"unknown", conntrack: bool = False,
                 send=None):
        self.table, self.writer, self.tls_names, self.k8s, self.net = table, writer, tls_names, k8s, net
        self.loki = LokiTable(writer, k8s, net, table)
        self.names = names if names is not None else np.zeros(0, dtype=INTF_NAME)
        self.agent_ip, self.unknown, self.conntrack, self.send = agent_ip, unknown, conntrack, send
        self.entries = self.batches = 0

    def ExportEvicted(self, raw, now_ns: int, mono_ns: int, time_received: int = 0, loki_now_ns: int = None, hash_ids=None, present=None, parts=None,
                      rows=None, netev_table=None):
        n = len(raw)
        if n == 0:
            return [], []
        mono = mono_ns & ((1 << 64) - 1)
        now = self.writer.now_of_call(loki_now_ns if loki_now_ns is not None else now_ns, time_received)
        if now is None:
            return [], list(range(n))
        ids = hash_ids
        if ids is None and self.conntrack:
            ids = self.table.conn_fold(raw, now_ns, mono, cap=min(n, L.CONN_MAX_CONNS), hash_ids=True)[3]
        rc, streams, groups, deferred, counts = loki_plan(self.table, raw, self.tls_names, self.k8s, self.net, self.loki, now_ns, mono, self.names,
                                                          self.agent_ip, time_received, self.unknown, ids, now, present=present, parts=parts, rows=rows,
                                                          netev_table=netev_table)
        rc, buf, boffs, bents = loki_write(self.table, self.loki.labels_of(streams), counts.n_batches)
        view = memoryview(np.ascontiguousarray(buf))
        bodies = [bytes(view[int(boffs[b]):int(boffs[b + 1])]) for b in range(counts.n_batches)]
        self.entries += int(bents.sum())
        self.batches += len(bodies)
        if self.send is not None:
            for body in bodies:
                self.send(body)
        return bodies, [int(i) for i in np.flatnonzero(deferred)]
