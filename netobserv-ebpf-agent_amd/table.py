"""FlowTable — object wrapper over one libnfagg handle (include/nfagg.h).

All computation happens in the HIP library; this file only marshals numpy
buffers and raw device pointers across the C ABI.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .records import FLOW_RECORD, ROLLUP_KINDS, FLOW_METRICS, INTF_NAME


class NfaggError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"nfagg error {code}: {msg}")
        self.code = code


class PinnedRecords:
    """Room for n 144-byte records in page-locked host memory (nfagg_host_alloc): `.records` is a numpy view. Buffers like this
    are sent to / filled by the GPU by DMA directly (include/nfagg.h nfagg_host_alloc); pageable arrays take one more host copy."""

    def __init__(self, n: int):
        p = C.c_void_p()
        rc = L.lib.nfagg_host_alloc(max(int(n), 1) * 144, C.byref(p))
        if rc != L.OK or not p:
            raise NfaggError(rc, "nfagg_host_alloc failed")
        self._p = p
        self.records = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(int(n), 1) * 144,)).view(FLOW_RECORD)[:n]

    def close(self):
        if self._p:
            self.records = None
            L.lib.nfagg_host_free(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _HostPoolInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("workers", C.c_uint32), ("parts", C.c_uint32), ("bound", C.c_uint32),
                ("numa_node", C.c_int32), ("pad_", C.c_uint32), ("calibrated_gbs", C.c_double)]


def host_threads(threads: int = 0, numa_node: int = -1) -> int:
    """nfagg_host_threads: (re)shape the process's copy workers; returns the workers running."""
    rc = L.lib.nfagg_host_threads(threads, numa_node)
    if rc < 0:
        raise NfaggError(rc, "nfagg_host_threads")
    return rc


def host_info() -> dict:
    """nfagg_host_info: workers, the calibrated number of parts per copy, NUMA binding, the calibration's best rate."""
    info = _HostPoolInfo(struct_size=C.sizeof(_HostPoolInfo))
    rc = L.lib.nfagg_host_info(C.byref(info))
    if rc != L.OK:
        raise NfaggError(rc, "nfagg_host_info")
    return {"workers": info.workers, "parts": info.parts, "bound": bool(info.bound), "numa_node": info.numa_node,
            "calibrated_GBs": round(info.calibrated_gbs, 1)}


def debug_live_buffers() -> int:
    """Device and page-locked allocations of the library alive in this process (testing aid: tests/test_lifecycle_gpu.py)."""
    return int(L.lib.nfagg_debug_live_buffers())


def device_numa_node(device: int = 0) -> int:
    return int(L.lib.nfagg_device_numa_node(device))


_ROLLUP_FN = {
    "additional": L.lib.nfagg_rollup_additional, "dns": L.lib.nfagg_rollup_dns, "drops": L.lib.nfagg_rollup_drops,
    "network_events": L.lib.nfagg_rollup_network_events, "xlat": L.lib.nfagg_rollup_xlat, "quic": L.lib.nfagg_rollup_quic,
}


class FlowTable:
    """The GPU-resident replacement of Accounter.entries (pkg/flow/account.go:22)."""

    def __init__(self, max_entries=5000, device=0, mode=L.MODE_ACCOUNTER, sketches=0, cm_depth=0, cm_log2_width=0,
                 hll_p=0, table_log2_slots=0, staging_records=0, n_shards=1, shard_id=0, profile=False,
                 ingest_variant=0, ext_sketch=None, copy_threads=0, local_fold=False):
        cfg = L.Config()
        cfg.struct_size = C.sizeof(L.Config)
        cfg.device = device
        cfg.max_entries = max_entries
        cfg.table_log2_slots = table_log2_slots
        cfg.mode = mode
        cfg.sketch_flags = sketches
        cfg.cm_depth, cfg.cm_log2_width, cfg.hll_p = cm_depth, cm_log2_width, hll_p
        cfg.staging_records = staging_records
        cfg.n_shards, cfg.shard_id = n_shards, shard_id
        cfg.profile = 1 if profile else 0
        cfg.ingest_variant = ingest_variant
        cfg.copy_threads = copy_threads
        cfg.local_fold = 1 if local_fold else 0       # a rank of a local-fold job (nfagg_partials_*); kernel-dedup mode: sub-flow table
        if ext_sketch:
            for k, p in enumerate(ext_sketch):
                cfg.ext_sketch[k] = p
        self._h = C.c_void_p()
        rc = L.lib.nfagg_create(C.byref(cfg), C.byref(self._h))
        if rc != L.OK:
            msg = L.lib.nfagg_last_error(None)
            self._h = None
            raise NfaggError(rc, msg.decode() if msg else "nfagg_create failed")
        self.max_entries = max_entries if max_entries else 5000

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            L.lib.nfagg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, ok=(L.OK,)):
        if rc not in ok:
            msg = L.lib.nfagg_last_error(self._h)
            raise NfaggError(rc, msg.decode() if msg else "")
        return rc

    # -- ingest
    def ingest(self, records: np.ndarray):
        """nfagg_ingest: fold host records in order. Returns (status, consumed)."""
        records = np.ascontiguousarray(records)
        assert records.dtype.itemsize == 144 or records.dtype == np.uint8
        n = records.nbytes // 144
        consumed = C.c_size_t(0)
        rc = L.lib.nfagg_ingest(self._h, records.ctypes.data_as(C.c_void_p), n, C.byref(consumed))
        self._check(rc, (L.OK, L.FULL))
        return rc, consumed.value

    def ingest_device(self, d_ptr: int, n: int):
        consumed = C.c_size_t(0)
        rc = L.lib.nfagg_ingest_device(self._h, C.c_void_p(d_ptr), n, C.byref(consumed))
        self._check(rc, (L.OK, L.FULL))
        return rc, consumed.value

    def staging_acquire(self):
        buf, cap = C.c_void_p(), C.c_size_t(0)
        self._check(L.lib.nfagg_staging_acquire(self._h, C.byref(buf), C.byref(cap)))
        arr = np.ctypeslib.as_array(C.cast(buf, C.POINTER(C.c_uint8)), shape=(cap.value * 144,)).view(FLOW_RECORD)
        return arr

    def staging_commit(self, n):
        consumed = C.c_size_t(0)
        rc = L.lib.nfagg_staging_commit(self._h, n, C.byref(consumed))
        self._check(rc, (L.OK, L.FULL))
        return rc, consumed.value

    def __len__(self):
        v = C.c_uint64(0)
        self._check(L.lib.nfagg_len(self._h, C.byref(v)))
        return v.value

    # -- evict
    def evict(self, reason=L.REASON_TIMEOUT, cap=None, out=None) -> np.ndarray:
        """nfagg_evict: every live flow as one flow_record_t; table cleared. out: a FLOW_RECORD array to deliver into (a caller
        that evicts tick after tick reuses one, as the cgo shim does)."""
        if out is not None:
            cap = len(out)
        elif cap is None:
            cap = max(len(self), 1)
        if out is None:
            out = np.empty(cap, dtype=FLOW_RECORD)
        n = C.c_size_t(0)
        rc = L.lib.nfagg_evict(self._h, reason, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
        self._check(rc, (L.OK, L.TRUNCATED))
        if rc == L.TRUNCATED:
            return self.evict(reason, cap=n.value)
        return out[: n.value]

    # -- account: the record arm with its evictions on "full" (account.go:81-96) in one call
    def account(self, records: np.ndarray, out_cap=None, max_epochs=None, out=None):
        """nfagg_account. Returns (status, consumed, epochs): epochs = list of arrays (views of `out`), one per eviction on
        "full", in order. out: a FLOW_RECORD array to deliver into (a caller that accounts batch after batch reuses one)."""
        records = np.ascontiguousarray(records)
        n = records.nbytes // 144
        if out is not None:
            out_cap = len(out)
        if out_cap is None:
            out_cap = max(n + self.max_entries, self.max_entries)        # every record may start a flow; plus what is live already
        if max_epochs is None:
            max_epochs = n // max(self.max_entries, 1) + 2
        if out is None:
            out = np.empty(max(out_cap, 1), dtype=FLOW_RECORD)
        ends = (C.c_uint64 * max(max_epochs, 1))()
        n_ep, consumed = C.c_size_t(0), C.c_size_t(0)
        rc = L.lib.nfagg_account(self._h, records.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p), out_cap, ends, max_epochs,
                                 C.byref(n_ep), C.byref(consumed))
        self._check(rc, (L.OK, L.TRUNCATED))
        epochs, lo = [], 0
        for e in range(n_ep.value):
            epochs.append(out[lo:int(ends[e])])
            lo = int(ends[e])
        return rc, consumed.value, epochs

    def account_device(self, d_ptr: int, n: int, d_out: int, out_cap: int, max_epochs: int):
        """nfagg_account_device. Returns (status, consumed, epoch_end list)."""
        ends = (C.c_uint64 * max(max_epochs, 1))()
        n_ep, consumed = C.c_size_t(0), C.c_size_t(0)
        rc = L.lib.nfagg_account_device(self._h, C.c_void_p(d_ptr), n, C.c_void_p(d_out or None), out_cap, ends, max_epochs, C.byref(n_ep), C.byref(consumed))
        self._check(rc, (L.OK, L.TRUNCATED))
        return rc, consumed.value, [int(ends[e]) for e in range(n_ep.value)]

    def evict_device(self, d_ptr: int, cap: int, reason=L.REASON_TIMEOUT) -> int:
        n = C.c_size_t(0)
        self._check(L.lib.nfagg_evict_device(self._h, reason, C.c_void_p(d_ptr), cap, C.byref(n)))
        return n.value

    # -- rollups (pkg/tracer/tracer.go:1057-1146)
    def rollup(self, kind: str, partials: np.ndarray, n_cpu: int, base: np.ndarray):
        dt = ROLLUP_KINDS[kind]
        partials = np.ascontiguousarray(partials, dtype=dt)
        n_flows = partials.size // n_cpu
        base = np.ascontiguousarray(base, dtype=FLOW_METRICS).copy()
        folded = np.zeros(n_flows, dtype=dt)
        self._check(_ROLLUP_FN[kind](self._h, partials.ctypes.data_as(C.c_void_p), n_flows, n_cpu,
                                     base.ctypes.data_as(C.c_void_p), folded.ctypes.data_as(C.c_void_p)))
        return base, folded

    # -- map merge (LookupAndDeleteMap's join), nfagg_map_merge
    _KIND_ORDER = ("additional", "dns", "drops", "network_events", "xlat", "quic")      # NFAGG_ROLLUP_*

    def map_merge(self, main_ids, main_vals, feats: dict, n_cpu: int, cap=None):
        """feats: {kind: (ids[n], partials[n, n_cpu])}. Returns (records, present, parts dict, n_duplicate_keys):
        one entry per merged flow, in order of first appearance."""
        mi = np.ascontiguousarray(main_ids, dtype=FLOW_RECORD["id"])
        mv = np.ascontiguousarray(main_vals, dtype=FLOW_METRICS)
        assert len(mi) == len(mv)
        keep = [mi, mv]
        main = L.MapView(mi.ctypes.data if len(mi) else None, mv.ctypes.data if len(mv) else None, len(mi))
        views = (L.MapView * 6)()
        total = len(mi)
        for k, name in enumerate(self._KIND_ORDER):
            if name not in feats:
                continue
            fi = np.ascontiguousarray(feats[name][0], dtype=FLOW_RECORD["id"])
            fv = np.ascontiguousarray(feats[name][1], dtype=ROLLUP_KINDS[name]).reshape(-1)
            assert fv.size == len(fi) * n_cpu, name
            keep += [fi, fv]
            views[k] = L.MapView(fi.ctypes.data if len(fi) else None, fv.ctypes.data if len(fi) else None, len(fi))
            total += len(fi)
        cap = total if cap is None else cap
        recs = np.zeros(max(cap, 1), dtype=FLOW_RECORD)
        present = np.zeros(max(cap, 1), dtype=np.uint8)
        parts = {name: np.zeros(max(cap, 1), dtype=ROLLUP_KINDS[name]) for name in self._KIND_ORDER}
        out = L.MergedFlows(recs.ctypes.data, present.ctypes.data, *[parts[name].ctypes.data for name in self._KIND_ORDER])
        n_out, n_dup = C.c_size_t(0), C.c_size_t(0)
        rc = L.lib.nfagg_map_merge(self._h, C.byref(main), views, n_cpu, C.byref(out), cap, C.byref(n_out), C.byref(n_dup))
        if rc == L.TRUNCATED:                      # caller's cap too small: retry with the size the library reported (as evict does)
            return self.map_merge(main_ids, main_vals, feats, n_cpu, cap=n_out.value)
        self._check(rc)
        n = n_out.value
        return recs[:n], present[:n], {k: v[:n] for k, v in parts.items()}, n_dup.value

    def map_merge_device(self, d_main, d_feats: dict, n_cpu: int, d_out: dict, cap: int):
        """Raw device pointers: d_main = (d_ids, d_vals, n); d_feats = {kind: (d_ids, d_vals, n)};
        d_out = {"records", "present", kind...: pointer}. Returns (rc, n_out, n_duplicate_keys)."""
        main = L.MapView(d_main[0] or None, d_main[1] or None, d_main[2])
        views = (L.MapView * 6)()
        for k, name in enumerate(self._KIND_ORDER):
            if name in d_feats:
                views[k] = L.MapView(d_feats[name][0] or None, d_feats[name][1] or None, d_feats[name][2])
        out = L.MergedFlows(d_out.get("records") or None, d_out.get("present") or None,
                            *[d_out.get(name) or None for name in self._KIND_ORDER])
        n_out, n_dup = C.c_size_t(0), C.c_size_t(0)
        rc = L.lib.nfagg_map_merge_device(self._h, C.byref(main), views, n_cpu, C.byref(out), cap, C.byref(n_out), C.byref(n_dup))
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        return rc, n_out.value, n_dup.value

    # -- sketches
    def sketch_snapshot(self, which):
        p, b = C.c_void_p(), C.c_size_t(0)
        self._check(L.lib.nfagg_sketch_device_ptr(self._h, which, C.byref(p), C.byref(b)))
        if which in (L.CM_SRC, L.CM_DST):
            out = np.zeros(b.value // 8, dtype=np.uint64)
        else:
            out = np.zeros(b.value, dtype=np.uint8)
        self._check(L.lib.nfagg_sketch_snapshot(self._h, which, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def sketch_device_ptr(self, which):
        p, b = C.c_void_p(), C.c_size_t(0)
        self._check(L.lib.nfagg_sketch_device_ptr(self._h, which, C.byref(p), C.byref(b)))
        return p.value, b.value

    def sketch_reset(self):
        self._check(L.lib.nfagg_sketch_reset(self._h))

    def hll_estimate(self, which):
        v = C.c_double(0)
        self._check(L.lib.nfagg_hll_estimate(self._h, which, C.byref(v)))
        return v.value

    def cm_query(self, which, ip16: bytes):
        v = C.c_uint64(0)
        buf = (C.c_uint8 * 16).from_buffer_copy(bytes(ip16))
        self._check(L.lib.nfagg_cm_query(self._h, which, buf, C.byref(v)))
        return v.value

    HEAVY_HITTER = np.dtype([("ip", "u1", 16), ("estimate", "<u8")])

    def cm_topk(self, which, records, k: int, device_ptr: int = 0, n: int = 0) -> np.ndarray:
        """nfagg_cm_topk: the k heaviest endpoints (Count-Min estimate) among the addresses of `records` (host array), or of
        the n records at device_ptr."""
        out = np.zeros(max(k, 1), dtype=self.HEAVY_HITTER)
        n_out = C.c_size_t(0)
        if device_ptr:
            rc = L.lib.nfagg_cm_topk_device(self._h, which, C.c_void_p(device_ptr), n, k, out.ctypes.data_as(C.c_void_p), C.byref(n_out))
        else:
            r = np.ascontiguousarray(records)
            rc = L.lib.nfagg_cm_topk(self._h, which, r.ctypes.data_as(C.c_void_p), r.nbytes // 144, k, out.ctypes.data_as(C.c_void_p), C.byref(n_out))
        self._check(rc)
        return out[: n_out.value]

    # -- misc
    # -- export encode (record -> protobuf), nfagg_encode_pb
    def _pb_options(self, now_unix_ns, mono_now_ns, agent_ip16, names, unknown):
        o, names = _encode_options(L.PbOptions, now_unix_ns, mono_now_ns, names, unknown)
        o.agent_ip[:] = list(bytes(agent_ip16))
        return o, names

    def _encode_grown(self, n, per_flow, call):
        """The host-memory encoders' output buffer: per_flow bytes per flow as a first guess; on TRUNCATED, the size the
        library reported. call(buf pointer, cap, need) -> rc. Returns the bytes written."""
        need = C.c_size_t(0)
        cap = max(per_flow * n, 64)
        while True:
            buf = np.zeros(cap, dtype=np.uint8)
            rc = call(buf.ctypes.data_as(C.c_void_p), cap, C.byref(need))
            if rc != L.TRUNCATED:
                self._check(rc)
                return buf[: need.value]
            cap = need.value

    @staticmethod
    def _pb_features(n, present, parts, device=False):
        """nfagg_pb_features from `present` (n bytes of FEAT_* bits) and parts = {"additional"|"dns"|"drops"|"xlat"|"quic":
        array of n structs}; with device=True the values are raw device pointers."""
        f = L.PbFeatures()
        f.struct_size = C.sizeof(L.PbFeatures)
        keep = []
        if device:
            f.present = present or None
            for k, v in parts.items():
                setattr(f, k, v or None)
            return f, keep
        p = np.ascontiguousarray(present, dtype=np.uint8)
        assert p.size == n
        keep.append(p)
        f.present = p.ctypes.data
        for k, v in parts.items():
            a = np.ascontiguousarray(v)
            assert a.dtype == ROLLUP_KINDS[k] and len(a) == n, k
            keep.append(a)
            setattr(f, k, a.ctypes.data)
        return f, keep

    @staticmethod
    def _content_parts(parts):
        return {k: v for k, v in (parts or {}).items() if k in _CONTENT_PARTS}

    def _pb(self, records, options, kafka_keys=False, features=None, rows=None, netev_table=None):
        """The host-memory entry points. options: _pb_options(...). features: (present, parts), present None: nfagg_encode_pb,
        else nfagg_encode_pb_content; with rows and netev_table nfagg_encode_pb_content_netev. Returns (buf, frame_offsets,
        body_len[, keys])."""
        r = np.ascontiguousarray(records)
        n = r.nbytes // 144
        o, keep = options
        head = (self._h, r.ctypes.data_as(C.c_void_p), n)
        fn, feat = L.lib.nfagg_encode_pb, None
        if features is not None and features[0] is not None:
            feat, keep_f = self._pb_features(n, features[0], self._content_parts(features[1]))
            fn, head = L.lib.nfagg_encode_pb_content, head + (C.byref(feat),)
        if netev_table is not None:
            assert feat is not None
            rw = np.ascontiguousarray(rows, dtype=np.uint16).reshape(n, 4)
            fn, head = L.lib.nfagg_encode_pb_content_netev, head + (rw.ctypes.data_as(C.c_void_p), netev_table._t)
        off = np.zeros(n + 1, dtype=np.uint64)
        blen = np.zeros(max(n, 1), dtype=np.uint32)
        keys = np.zeros((max(n, 1), 32), dtype=np.uint8) if kafka_keys else None
        buf = self._encode_grown(n, 256, lambda p, cap, need: fn(
            *head, C.byref(o), p, cap, off.ctypes.data_as(C.c_void_p), blen.ctypes.data_as(C.c_void_p),
            keys.ctypes.data_as(C.c_void_p) if kafka_keys else None, need))
        out = (buf, off, blen[:n])
        return out + (keys[:n],) if kafka_keys else out

    def _pb_device(self, d_records, n, options, d_out, out_cap, d_frame_offsets, d_body_len, d_kafka_keys=0, features=None, d_rows=0,
                   netev_table=None):
        """The device entry points (raw device pointers); the optionals select as in _pb, features = (d_present, d_parts).
        Returns (rc, bytes needed/written)."""
        o, keep = options
        need = C.c_size_t(0)
        head = (self._h, C.c_void_p(d_records), n)
        fn, feat = L.lib.nfagg_encode_pb_device, None
        if features is not None:
            feat, _ = self._pb_features(n, features[0], self._content_parts(features[1]), device=True)
            fn, head = L.lib.nfagg_encode_pb_content_device, head + (C.byref(feat),)
        if netev_table is not None:
            assert feat is not None
            fn, head = L.lib.nfagg_encode_pb_content_netev_device, head + (C.c_void_p(d_rows or None), netev_table._t)
        rc = fn(*head, C.byref(o), C.c_void_p(d_out or None), out_cap, C.c_void_p(d_frame_offsets), C.c_void_p(d_body_len),
                C.c_void_p(d_kafka_keys or None), C.byref(need))
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        return rc, need.value

    def encode_pb(self, records: np.ndarray, now_unix_ns: int, mono_now_ns: int, agent_ip16: bytes, names: np.ndarray,
                  unknown: bytes = b"unknown", kafka_keys=False, present=None, parts=None):
        """FlowsToPB + proto.Marshal of evicted records on the GPU. Returns (buf, frame_offsets, body_len[, keys]):
        buf[frame_offsets[a]:frame_offsets[b]] is a serialized pbflow.Records of entries a..b-1; the last body_len[i]
        bytes of frame i are the serialized pbflow.Record. With present/parts (see _pb_features) the flows are full
        BpfFlowContents of the MapTracer branch (nfagg_encode_pb_content)."""
        return self._pb(records, self._pb_options(now_unix_ns, mono_now_ns, agent_ip16, names, unknown), kafka_keys, (present, parts))

    def encode_pb_device(self, d_records: int, n: int, now_unix_ns: int, mono_now_ns: int, agent_ip16: bytes, names: np.ndarray,
                         d_out: int, out_cap: int, d_frame_offsets: int, d_body_len: int, d_kafka_keys: int = 0,
                         unknown: bytes = b"unknown", d_present: int = 0, d_parts=None):
        """Device-resident variant (raw device pointers). Returns (rc, bytes needed/written)."""
        return self._pb_device(d_records, n, self._pb_options(now_unix_ns, mono_now_ns, agent_ip16, names, unknown), d_out, out_cap,
                               d_frame_offsets, d_body_len, d_kafka_keys, (d_present, d_parts) if d_present else None)

    # -- export encode (record -> IPFIX messages), nfagg_encode_ipfix
    def encode_ipfix(self, records: np.ndarray, now_unix_ns: int, mono_now_ns: int, names: np.ndarray, export_time_s: int,
                     seq0: int, unknown: bytes = b"unknown", obs_domain_id: int = 1):
        """IPFIX.ExportFlows' messages for evicted records, encoded on the GPU (one message per flow, template v6 iff
        eth_protocol == 0x86DD). Returns (buf, msg_offsets): message i is buf[msg_offsets[i]:msg_offsets[i + 1]] and
        carries sequence number seq0 + i (mod 2**32); every message has Export Time export_time_s."""
        r = np.ascontiguousarray(records)
        n = r.nbytes // 144
        o, keep = ipfix_options(now_unix_ns, mono_now_ns, names, export_time_s, seq0, unknown, obs_domain_id)
        off = np.zeros(n + 1, dtype=np.uint64)
        buf = self._encode_grown(n, 120, lambda p, cap, need: L.lib.nfagg_encode_ipfix(
            self._h, r.ctypes.data_as(C.c_void_p), n, C.byref(o), p, cap, off.ctypes.data_as(C.c_void_p), need))
        return buf, off

    def encode_ipfix_device(self, d_records: int, n: int, now_unix_ns: int, mono_now_ns: int, names: np.ndarray, export_time_s: int,
                            seq0: int, d_out: int, out_cap: int, d_msg_offsets: int, unknown: bytes = b"unknown", obs_domain_id: int = 1):
        """Device-resident variant (raw device pointers; d_out = 0 asks for the size). Returns (rc, bytes needed/written)."""
        o, keep = ipfix_options(now_unix_ns, mono_now_ns, names, export_time_s, seq0, unknown, obs_domain_id)
        need = C.c_size_t(0)
        rc = L.lib.nfagg_encode_ipfix_device(self._h, C.c_void_p(d_records), n, C.byref(o), C.c_void_p(d_out or None), out_cap,
                                             C.c_void_p(d_msg_offsets), C.byref(need))
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        return rc, need.value

    # -- export encode (record -> direct-FLP JSON lines), nfagg_encode_flp_json*
    def _flp_json(self, records, options, features=None, rows=None, netev_table=None, tls_names=None, k8s=None, net=None, hash_ids=None):
        """The host-memory entry points. options: flp_options(...). features: None (nfagg_encode_flp_json) or (present, parts)
        (the *_content ones; present None: no flow carries a part). rows and netev_table: the *_netev one. tls_names:
        nfagg_encode_flp_json_tls, which takes the others as options and defers nothing; k8s (with tls_names): nfagg_encode_flp_json_k8s;
        net (with k8s): nfagg_encode_flp_json_net; hash_ids (with net): nfagg_encode_flp_json_conn. Returns (buf, line_offsets, deferred)."""
        r = np.ascontiguousarray(records)
        n = r.nbytes // 144
        o, keep = options
        feat = None
        if features is not None and features[0] is not None:
            feat, keep_f = self._pb_features(n, features[0], self._content_parts(features[1]))
        rw = np.ascontiguousarray(rows, dtype=np.uint16).reshape(n, 4) if rows is not None else None
        off = np.zeros(n + 1, dtype=np.uint64)
        deferred = np.zeros(n, dtype=np.uint8)
        n_def = C.c_size_t(0)
        head = (self._h, r.ctypes.data_as(C.c_void_p), n)
        f_arg = (C.byref(feat) if feat is not None else None,)
        ne_args = (rw.ctypes.data_as(C.c_void_p) if rw is not None else None, netev_table._t if netev_table is not None else None)
        if tls_names is not None:
            fn, head, flags = L.lib.nfagg_encode_flp_json_tls, head + f_arg + ne_args + (tls_names._t,), ()
            if k8s is not None:
                fn, head = L.lib.nfagg_encode_flp_json_k8s, head + (k8s._t,)
                if net is not None:
                    fn, head = L.lib.nfagg_encode_flp_json_net, head + (net._t,)
                    if hash_ids is not None:
                        ids = np.ascontiguousarray(hash_ids, dtype=np.uint64)
                        assert ids.size == n
                        fn, head = L.lib.nfagg_encode_flp_json_conn, head + (ids.ctypes.data_as(C.c_void_p) if n else None,)
        else:
            flags = (deferred.ctypes.data_as(C.c_void_p), C.byref(n_def))
            if netev_table is not None:
                fn, head = L.lib.nfagg_encode_flp_json_content_netev, head + f_arg + ne_args
            elif features is not None:
                fn, head = L.lib.nfagg_encode_flp_json_content, head + f_arg
            else:
                fn = L.lib.nfagg_encode_flp_json
        per_flow = 448 if fn is L.lib.nfagg_encode_flp_json else 1024 if k8s is not None else 640
        buf = self._encode_grown(n, per_flow, lambda p, cap, need: fn(*head, C.byref(o), p, cap, off.ctypes.data_as(C.c_void_p), *flags, need))
        assert int(deferred.sum()) == n_def.value
        return buf, off, deferred

    def _flp_json_device(self, d_records, n, options, d_out, out_cap, d_line_offsets, d_deferred=0, features=None, d_rows=0,
                         netev_table=None, tls_names=None, k8s=None, net=None, d_hash_ids=None):
        """The device entry points (raw device pointers); the optionals select as in _flp_json, features = (d_present, d_parts).
        Returns (rc, bytes needed/written, deferred records)."""
        o, keep = options
        feat = None
        if features is not None:
            feat, _ = self._pb_features(n, features[0], self._content_parts(features[1]), device=True)
        need, n_def = C.c_size_t(0), C.c_size_t(0)
        head = (self._h, C.c_void_p(d_records or None), n)
        f_arg = (C.byref(feat) if feat is not None else None,)
        ne_args = (C.c_void_p(d_rows or None), netev_table._t if netev_table is not None else None)
        flags = (C.c_void_p(d_deferred or None), C.byref(n_def))
        if tls_names is not None:
            fn, head, flags = L.lib.nfagg_encode_flp_json_tls_device, head + f_arg + ne_args + (tls_names._t,), ()
            if k8s is not None:
                fn, head = L.lib.nfagg_encode_flp_json_k8s_device, head + (k8s._t,)
                if net is not None:
                    fn, head = L.lib.nfagg_encode_flp_json_net_device, head + (net._t,)
                    if d_hash_ids is not None:
                        fn, head = L.lib.nfagg_encode_flp_json_conn_device, head + (C.c_void_p(d_hash_ids or None),)
        elif netev_table is not None:
            fn, head = L.lib.nfagg_encode_flp_json_content_netev_device, head + f_arg + ne_args
        elif features is not None:
            fn, head = L.lib.nfagg_encode_flp_json_content_device, head + f_arg
        else:
            fn = L.lib.nfagg_encode_flp_json_device
        rc = fn(*head, C.byref(o), C.c_void_p(d_out or None), out_cap, C.c_void_p(d_line_offsets or None), *flags, C.byref(need))
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        return rc, need.value, n_def.value

    def encode_flp_json(self, records: np.ndarray, now_unix_ns: int, mono_now_ns: int, names: np.ndarray, agent_ip=None,
                        time_received: int = 0, unknown: bytes = b"unknown"):
        """The direct-FLP stdout lines (`format: json`, keys sorted) for evicted records, encoded on the GPU. agent_ip: 16 (or
        4) bytes, None = a nil AgentIP ("<nil>"). Returns (buf, line_offsets, deferred): line i is
        buf[line_offsets[i]:line_offsets[i + 1]], its newline included; deferred[i] == 1 marks a record that carries TLS
        version / cipher suite / key share, whose line is empty and which the caller formats itself."""
        return self._flp_json(records, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown))

    def encode_flp_json_device(self, d_records: int, n: int, now_unix_ns: int, mono_now_ns: int, names: np.ndarray, agent_ip,
                               time_received: int, d_out: int, out_cap: int, d_line_offsets: int, d_deferred: int = 0,
                               unknown: bytes = b"unknown"):
        """Device-resident variant (raw device pointers; d_out = 0 asks for the size, d_deferred = 0: no flags wanted).
        Returns (rc, bytes needed/written, deferred records)."""
        return self._flp_json_device(d_records, n, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown),
                                     d_out, out_cap, d_line_offsets, d_deferred)

    # -- export encode (MapTracer flow -> direct-FLP JSON line), nfagg_encode_flp_json_content
    def encode_flp_json_content(self, records: np.ndarray, present, parts, now_unix_ns: int, mono_now_ns: int, names: np.ndarray,
                                agent_ip=None, time_received: int = 0, unknown: bytes = b"unknown"):
        """encode_flp_json over full BpfFlowContents: `records`, `present` (FEAT_* bits per flow) and `parts` ({"additional" |
        "dns" | "drops" | "xlat" | "quic": array of n structs}; other kinds are ignored) as map_merge returns them.
        present=None: no flow carries a part. Returns (buf, line_offsets, deferred) as encode_flp_json does."""
        return self._flp_json(records, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown), (present, parts))

    def encode_flp_json_content_device(self, d_records: int, n: int, d_present: int, d_parts, now_unix_ns: int, mono_now_ns: int,
                                       names: np.ndarray, agent_ip, time_received: int, d_out: int, out_cap: int, d_line_offsets: int,
                                       d_deferred: int = 0, unknown: bytes = b"unknown"):
        """Device-resident variant (raw device pointers, e.g. the d_out of map_merge_device; d_present = 0: no parts; d_out = 0
        asks for the size). Returns (rc, bytes needed/written, deferred records)."""
        return self._flp_json_device(d_records, n, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown),
                                     d_out, out_cap, d_line_offsets, d_deferred, (d_present, d_parts) if d_present else None)

    # -- network events (nfagg_netev_*): the decoder's answers as a table, the per-flow work on the GPU
    def netev_table(self, entries) -> "NetevTable":
        """A cookie table on this handle's device; entries: [(cookie8, event)], see NetevTable."""
        return NetevTable(entries, self)

    def netev_resolve(self, table: "NetevTable", present, network_events, drops=None, missing_cap: int = 1024):
        """record.go:126-157 for every flow (nfagg_netev_resolve): present / network_events / drops as map_merge returns them
        (drops=None: no flow has a drops part). Returns (present_out, drops_out, rows uint16[n, 4], missing cookies (list of
        8-byte strings, distinct, order unspecified), overflow)."""
        p = np.ascontiguousarray(present, dtype=np.uint8)
        n = p.size
        ne = np.ascontiguousarray(network_events, dtype=ROLLUP_KINDS["network_events"]) if network_events is not None else None
        dr = np.ascontiguousarray(drops, dtype=ROLLUP_KINDS["drops"]) if drops is not None else None
        assert (ne is None or len(ne) == n) and (dr is None or len(dr) == n)
        p_out = np.zeros(n, dtype=np.uint8)
        d_out = np.zeros(n, dtype=ROLLUP_KINDS["drops"])
        rows = np.zeros((n, 4), dtype=np.uint16)
        miss = np.zeros((max(missing_cap, 1), 8), dtype=np.uint8)
        n_miss, over = C.c_size_t(0), C.c_int(0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        self._check(L.lib.nfagg_netev_resolve(self._h, table._t, ptr(p), ptr(ne), ptr(dr), n, ptr(p_out), ptr(d_out), ptr(rows),
                                              miss.ctypes.data_as(C.c_void_p), missing_cap, C.byref(n_miss), C.byref(over)))
        return p_out, d_out, rows, [miss[k].tobytes() for k in range(n_miss.value)], bool(over.value)

    def netev_resolve_device(self, table: "NetevTable", d_present: int, d_network_events: int, d_drops: int, n: int, d_present_out: int,
                             d_drops_out: int, d_rows_out: int, d_missing_set: int = 0, missing_cap: int = 0):
        """Device-resident variant (raw device pointers; outputs may alias the inputs). Returns (distinct missing cookies
        recorded, the all-zero cookie was missing, overflow); d_missing_set holds the non-zero ones, 0 = empty slot."""
        n_miss, zero, over = C.c_size_t(0), C.c_int(0), C.c_int(0)
        self._check(L.lib.nfagg_netev_resolve_device(
            self._h, table._t, C.c_void_p(d_present or None), C.c_void_p(d_network_events or None), C.c_void_p(d_drops or None), n,
            C.c_void_p(d_present_out or None), C.c_void_p(d_drops_out or None), C.c_void_p(d_rows_out or None),
            C.c_void_p(d_missing_set or None), missing_cap, C.byref(n_miss), C.byref(zero), C.byref(over)))
        return n_miss.value, bool(zero.value), bool(over.value)

    def encode_pb_netev(self, records: np.ndarray, present, parts, rows, table: "NetevTable", now_unix_ns: int, mono_now_ns: int,
                        agent_ip16: bytes, names: np.ndarray, unknown: bytes = b"unknown"):
        """encode_pb with present/parts plus the flows' network events (nfagg_encode_pb_content_netev): present and
        parts["drops"] are netev_resolve's outputs, rows its rows. Returns (buf, frame_offsets, body_len)."""
        return self._pb(records, self._pb_options(now_unix_ns, mono_now_ns, agent_ip16, names, unknown), False, (present, parts), rows, table)

    def encode_pb_netev_device(self, d_records: int, n: int, d_present: int, d_parts, d_rows: int, table: "NetevTable", now_unix_ns: int,
                               mono_now_ns: int, agent_ip16: bytes, names: np.ndarray, d_out: int, out_cap: int, d_frame_offsets: int,
                               d_body_len: int, unknown: bytes = b"unknown"):
        """Device-resident variant (raw device pointers). Returns (rc, bytes needed/written)."""
        return self._pb_device(d_records, n, self._pb_options(now_unix_ns, mono_now_ns, agent_ip16, names, unknown), d_out, out_cap,
                               d_frame_offsets, d_body_len, 0, (d_present, d_parts), d_rows, table)

    def encode_flp_json_netev(self, records: np.ndarray, present, parts, rows, table: "NetevTable", now_unix_ns: int, mono_now_ns: int,
                              names: np.ndarray, agent_ip=None, time_received: int = 0, unknown: bytes = b"unknown"):
        """encode_flp_json_content plus the flows' network events (nfagg_encode_flp_json_content_netev); inputs as
        encode_pb_netev. Returns (buf, line_offsets, deferred)."""
        return self._flp_json(records, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown), (present, parts),
                              rows, table)

    def encode_flp_json_netev_device(self, d_records: int, n: int, d_present: int, d_parts, d_rows: int, table: "NetevTable",
                                     now_unix_ns: int, mono_now_ns: int, names: np.ndarray, agent_ip, time_received: int, d_out: int,
                                     out_cap: int, d_line_offsets: int, d_deferred: int = 0, unknown: bytes = b"unknown"):
        """Device-resident variant (raw device pointers). Returns (rc, bytes needed/written, deferred records)."""
        return self._flp_json_device(d_records, n, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown),
                                     d_out, out_cap, d_line_offsets, d_deferred, (d_present, d_parts), d_rows, table)

    # -- TLS names (nfagg_tls_names_*) and the direct-FLP encoder that writes them, nfagg_encode_flp_json_tls
    def tls_names(self, entries=None) -> "TlsNames":
        """A TLS name table on this handle's device; entries: [(kind, id, name)], default GO_TLS_NAMES. See TlsNames."""
        return TlsNames(GO_TLS_NAMES if entries is None else entries, self)

    def encode_flp_json_tls(self, records: np.ndarray, tls_names: "TlsNames", now_unix_ns: int, mono_now_ns: int, names: np.ndarray,
                            agent_ip=None, time_received: int = 0, unknown: bytes = b"unknown", present=None, parts=None, rows=None,
                            netev_table: "NetevTable" = None):
        """encode_flp_json (present=None), encode_flp_json_content (present / parts) or encode_flp_json_netev (rows and
        netev_table as well) with TLSVersion, TLSCipherSuite and TLSGroup written from `tls_names` (nfagg_encode_flp_json_tls):
        no record is deferred. Returns (buf, line_offsets)."""
        return self._flp_json(records, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown), (present, parts),
                              rows, netev_table, tls_names)[:2]

    def encode_flp_json_tls_device(self, d_records: int, n: int, tls_names: "TlsNames", now_unix_ns: int, mono_now_ns: int,
                                   names: np.ndarray, agent_ip, time_received: int, d_out: int, out_cap: int, d_line_offsets: int,
                                   unknown: bytes = b"unknown", d_present: int = 0, d_parts=None, d_rows: int = 0,
                                   netev_table: "NetevTable" = None):
        """Device-resident variant (raw device pointers; d_present = 0: no parts; d_out = 0 asks for the size). Returns (rc,
        bytes needed/written)."""
        return self._flp_json_device(d_records, n, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown),
                                     d_out, out_cap, d_line_offsets, 0, (d_present, d_parts) if d_present else None, d_rows, netev_table,
                                     tls_names)[:2]

    # -- Kubernetes enrichment (nfagg_k8s_*): the informers' answers as a table, the hash join and the keys on the GPU
    def k8s_table(self, entries, layer=None) -> "K8sTable":
        """A Kubernetes table on this handle's device; entries and layer as K8sTable takes them."""
        return K8sTable(entries, layer, self)

    def k8s_resolve(self, table: "K8sTable", records: np.ndarray) -> np.ndarray:
        """nfagg_k8s_resolve: uint32[n, 2], the table rows of each record's src_ip and dst_ip (L.K8S_NO_ROW: none; both for
        a record that is not IP)."""
        r = np.ascontiguousarray(records)
        n = r.nbytes // 144
        rows = np.zeros((n, 2), dtype=np.uint32)
        self._check(L.lib.nfagg_k8s_resolve(self._h, table._t, r.ctypes.data_as(C.c_void_p) if n else None, n,
                                            rows.ctypes.data_as(C.c_void_p) if n else None))
        return rows

    def k8s_resolve_device(self, table: "K8sTable", d_records: int, n: int, d_rows: int) -> None:
        """Device-resident variant (raw device pointers; d_rows: 2n uint32)."""
        self._check(L.lib.nfagg_k8s_resolve_device(self._h, table._t, C.c_void_p(d_records or None), n, C.c_void_p(d_rows or None)))

    def encode_flp_json_k8s(self, records: np.ndarray, tls_names: "TlsNames", k8s: "K8sTable", now_unix_ns: int, mono_now_ns: int,
                            names: np.ndarray, agent_ip=None, time_received: int = 0, unknown: bytes = b"unknown", present=None, parts=None,
                            rows=None, netev_table: "NetevTable" = None):
        """encode_flp_json_tls plus the Kubernetes keys of both endpoints and, for a table with a layer, K8S_FlowLayer
        (nfagg_encode_flp_json_k8s). Returns (buf, line_offsets)."""
        return self._flp_json(records, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown), (present, parts),
                              rows, netev_table, tls_names, k8s)[:2]

    def encode_flp_json_k8s_device(self, d_records: int, n: int, tls_names: "TlsNames", k8s: "K8sTable", now_unix_ns: int, mono_now_ns: int,
                                   names: np.ndarray, agent_ip, time_received: int, d_out: int, out_cap: int, d_line_offsets: int,
                                   unknown: bytes = b"unknown", d_present: int = 0, d_parts=None, d_rows: int = 0,
                                   netev_table: "NetevTable" = None):
        """Device-resident variant (raw device pointers; d_present = 0: no parts; d_out = 0 asks for the size). Returns (rc,
        bytes needed/written)."""
        return self._flp_json_device(d_records, n, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown),
                                     d_out, out_cap, d_line_offsets, 0, (d_present, d_parts) if d_present else None, d_rows, netev_table,
                                     tls_names, k8s)[:2]

    # -- direction, subnet labels, TCP flag names (nfagg_net_*): three more rules of the transform network stage
    def net_table(self, flags: int = 0, categories=()) -> "NetTable":
        """A net table on this handle's device; flags and categories as NetTable takes them."""
        return NetTable(flags, categories, self)

    def net_resolve(self, net: "NetTable", records: np.ndarray, k8s: "K8sTable" = None, k8s_rows: np.ndarray = None, agent_ip=None) -> np.ndarray:
        """nfagg_net_resolve: NET_ROW[n] (src_label, dst_label: L.NET_NO_LABEL for none; direction: L.NET_NO_DIRECTION for no
        key). k8s, k8s_rows (what k8s_resolve returned) and agent_ip (None: nil) are read for reinterpret_direction only."""
        r = np.ascontiguousarray(records)
        n = r.nbytes // 144
        out = np.zeros(n, dtype=NET_ROW)
        kr = np.ascontiguousarray(k8s_rows, dtype=np.uint32) if k8s_rows is not None else None
        o, keep = flp_options(agent_ip=agent_ip)
        self._check(L.lib.nfagg_net_resolve(self._h, net._t, k8s._t if k8s is not None else None, r.ctypes.data_as(C.c_void_p) if n else None, n,
                                            kr.ctypes.data_as(C.c_void_p) if kr is not None and n else None, C.byref(o),
                                            out.ctypes.data_as(C.c_void_p) if n else None))
        return out

    def net_resolve_device(self, net: "NetTable", d_records: int, n: int, d_out: int, k8s: "K8sTable" = None, d_k8s_rows: int = 0, agent_ip=None) -> None:
        """Device-resident variant (raw device pointers; d_out: n NET_ROW of 8 bytes)."""
        o, keep = flp_options(agent_ip=agent_ip)
        self._check(L.lib.nfagg_net_resolve_device(self._h, net._t, k8s._t if k8s is not None else None, C.c_void_p(d_records or None), n,
                                                   C.c_void_p(d_k8s_rows or None), C.byref(o), C.c_void_p(d_out or None)))

    def encode_flp_json_net(self, records: np.ndarray, tls_names: "TlsNames", k8s: "K8sTable", net: "NetTable", now_unix_ns: int, mono_now_ns: int,
                            names: np.ndarray, agent_ip=None, time_received: int = 0, unknown: bytes = b"unknown", present=None, parts=None,
                            rows=None, netev_table: "NetevTable" = None):
        """encode_flp_json_k8s plus the rules switched on in `net`: FlowDirection, SrcSubnetLabel / DstSubnetLabel, the names
        of the TCP flags as the value of Flags (nfagg_encode_flp_json_net). Returns (buf, line_offsets)."""
        return self._flp_json(records, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown), (present, parts),
                              rows, netev_table, tls_names, k8s, net)[:2]

    def encode_flp_json_net_device(self, d_records: int, n: int, tls_names: "TlsNames", k8s: "K8sTable", net: "NetTable", now_unix_ns: int,
                                   mono_now_ns: int, names: np.ndarray, agent_ip, time_received: int, d_out: int, out_cap: int,
                                   d_line_offsets: int, unknown: bytes = b"unknown", d_present: int = 0, d_parts=None, d_rows: int = 0,
                                   netev_table: "NetevTable" = None):
        """Device-resident variant (raw device pointers; d_present = 0: no parts; d_out = 0 asks for the size). Returns (rc,
        bytes needed/written)."""
        return self._flp_json_device(d_records, n, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown),
                                     d_out, out_cap, d_line_offsets, 0, (d_present, d_parts) if d_present else None, d_rows, netev_table,
                                     tls_names, k8s, net)[:2]

    # -- extract conntrack's flow logs (nfagg_encode_flp_json_conn): the *_net line with _HashId and _RecordType
    def encode_flp_json_conn(self, records: np.ndarray, tls_names: "TlsNames", k8s: "K8sTable", net: "NetTable", hash_ids: np.ndarray,
                             now_unix_ns: int, mono_now_ns: int, names: np.ndarray, agent_ip=None, time_received: int = 0,
                             unknown: bytes = b"unknown", present=None, parts=None, rows=None, netev_table: "NetevTable" = None):
        """encode_flp_json_net as extract conntrack emits its flow logs (nfagg_encode_flp_json_conn): a flow the stage does not
        track (no IP ethertype, or a protocol other than 6, 17, 132) has an empty line, every other line ends in
        "_HashId":"<hex of hash_ids[i]>","_RecordType":"flowLog". hash_ids: uint64[n], what conn_fold returned for these
        records. Returns (buf, line_offsets)."""
        return self._flp_json(records, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown), (present, parts),
                              rows, netev_table, tls_names, k8s, net, hash_ids)[:2]

    def encode_flp_json_conn_device(self, d_records: int, n: int, tls_names: "TlsNames", k8s: "K8sTable", net: "NetTable", d_hash_ids: int,
                                    now_unix_ns: int, mono_now_ns: int, names: np.ndarray, agent_ip, time_received: int, d_out: int,
                                    out_cap: int, d_line_offsets: int, unknown: bytes = b"unknown", d_present: int = 0, d_parts=None,
                                    d_rows: int = 0, netev_table: "NetevTable" = None):
        """Device-resident variant (raw device pointers; d_hash_ids: the d_hash_ids of conn_fold_device; d_present = 0: no
        parts; d_out = 0 asks for the size). Returns (rc, bytes needed/written)."""
        return self._flp_json_device(d_records, n, flp_options(now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown),
                                     d_out, out_cap, d_line_offsets, 0, (d_present, d_parts) if d_present else None, d_rows, netev_table,
                                     tls_names, k8s, net, d_hash_ids)[:2]

    # -- extract conntrack's conversation records (nfagg_encode_conn_json): one JSON line per conversation
    def conn_layout(self, fields) -> "ConnLayout":
        """A ConnLayout on this handle's device; fields as ConnLayout takes them."""
        return ConnLayout(fields, self)

    def encode_conn_json(self, carriers: np.ndarray, values: np.ndarray, layout: "ConnLayout", k8s: "K8sTable", net: "NetTable"):
        """The conversation records' lines (nfagg_encode_conn_json). carriers: FLOW_RECORD[n] with the connections' keys; values:
        CONN_VALUES[n]. Returns (buf, line_offsets, deferred): deferred[i] == 1 marks a conversation with an aggregate of
        magnitude >= 2^53, whose line is empty and which the caller formats itself."""
        r = np.ascontiguousarray(carriers)
        v = np.ascontiguousarray(values, dtype=CONN_VALUES)
        n = r.nbytes // 144
        assert v.size == n
        off, deferred, n_def = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint8), C.c_size_t(0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if n else None  # noqa: E731
        buf = self._encode_grown(n, 1024, lambda p, cap, need: L.lib.nfagg_encode_conn_json(
            self._h, ptr(r), ptr(v), n, layout._t, k8s._t, net._t, p, cap, off.ctypes.data_as(C.c_void_p), ptr(deferred), C.byref(n_def), need))
        assert int(deferred.sum()) == n_def.value
        return buf, off, deferred

    def encode_conn_json_device(self, d_carriers: int, d_values: int, n: int, layout: "ConnLayout", k8s: "K8sTable", net: "NetTable", d_out: int,
                                out_cap: int, d_line_offsets: int, d_deferred: int = 0):
        """Device-resident variant (raw device pointers; d_out = 0 asks for the size). Returns (rc, bytes needed/written, deferred)."""
        need, n_def = C.c_size_t(0), C.c_size_t(0)
        rc = L.lib.nfagg_encode_conn_json_device(self._h, C.c_void_p(d_carriers or None), C.c_void_p(d_values or None), n, layout._t, k8s._t, net._t,
                                                 C.c_void_p(d_out or None), out_cap, C.c_void_p(d_line_offsets or None), C.c_void_p(d_deferred or None),
                                                 C.byref(n_def), C.byref(need))
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        return rc, need.value, n_def.value

    # -- flow metrics (nfagg_metrics_*): the GROUP BY under the `encode prom` counters
    def metrics_table(self, k8s: "K8sTable", groupings) -> "MetricsTable":
        """A metrics table on this handle's device; groupings: the dimension masks (L.DIM_*), at most L.MET_MAX_GROUPINGS."""
        return MetricsTable(k8s, groupings, self)

    def metrics_fold(self, met: "MetricsTable", records: np.ndarray, k8s_rows: np.ndarray, net_rows: np.ndarray = None, caps=4096):
        """nfagg_metrics_fold: k8s_rows / net_rows are what k8s_resolve / net_resolve returned for these records (net_rows may be
        None when no grouping selects a label or the direction). caps: one cap, or one per grouping. Returns (rc, groups,
        n_groups): groups[g] is a METRIC_GROUP array in unspecified order; with rc == L.TRUNCATED every groups[g] is empty and
        n_groups[g] is exact for the groupings that fit and a lower bound above the cap for the others."""
        r = np.ascontiguousarray(records)
        n = r.nbytes // 144
        G = len(met.groupings)
        caps = [int(caps)] * G if np.isscalar(caps) else [int(c) for c in caps]
        kr = np.ascontiguousarray(k8s_rows, dtype=np.uint32)
        nr = np.ascontiguousarray(net_rows, dtype=NET_ROW) if net_rows is not None else None
        outs = [np.zeros(min(c, L.MET_MAX_GROUPS), dtype=METRIC_GROUP) for c in caps]
        ptrs = (C.c_void_p * G)(*[o.ctypes.data if o.size else None for o in outs])
        cap_a, n_a = (C.c_uint32 * G)(*caps), (C.c_uint32 * G)()
        rc = L.lib.nfagg_metrics_fold(self._h, met._t, r.ctypes.data_as(C.c_void_p) if n else None, n, kr.ctypes.data_as(C.c_void_p) if n else None,
                                      nr.ctypes.data_as(C.c_void_p) if nr is not None and n else None, cap_a, ptrs, n_a)
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        counts = [int(x) for x in n_a]
        return rc, [o[:c if rc == L.OK else 0] for o, c in zip(outs, counts)], counts

    def metrics_fold_device(self, met: "MetricsTable", d_records: int, n: int, d_k8s_rows: int, d_net_rows: int, caps, d_outs):
        """Device-resident variant (raw device pointers; d_net_rows = 0: none; d_outs[g]: room for caps[g] groups of 64 bytes,
        16-byte aligned). Returns (rc, n_groups)."""
        G = len(met.groupings)
        ptrs = (C.c_void_p * G)(*[p or None for p in d_outs])
        cap_a, n_a = (C.c_uint32 * G)(*[int(c) for c in caps]), (C.c_uint32 * G)()
        rc = L.lib.nfagg_metrics_fold_device(self._h, met._t, C.c_void_p(d_records or None), n, C.c_void_p(d_k8s_rows or None),
                                             C.c_void_p(d_net_rows or None), cap_a, ptrs, n_a)
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        return rc, [int(x) for x in n_a]

    def metrics_table_specs(self, k8s: "K8sTable", specs) -> "MetricsTable":
        """A metrics table of specs (dicts of dims, xdims, value, hist, bounds: MetricsTable.spec) on this handle's device, for
        metrics_fold_content."""
        return MetricsTable(k8s, None, self, specs=specs)

    def _fold_content_args(self, met, caps):
        G = len(met.groupings)
        caps = [int(caps)] * G if np.isscalar(caps) else [int(c) for c in caps]
        return G, caps, (C.c_uint32 * G)(*caps), (C.c_uint32 * G)()

    def metrics_fold_content(self, met: "MetricsTable", records: np.ndarray, k8s_rows: np.ndarray, net_rows: np.ndarray = None, caps=4096, features=None):
        """nfagg_metrics_fold_content: metrics_fold over a table of specs (or a plain one) and the flows' feature parts.
        features: (present, parts) as map_merge returns and encode_flp_json_content takes them, or None: no flow has a part.
        Returns (rc, groups, n_groups) with METRIC_GROUP_CONTENT arrays."""
        r = np.ascontiguousarray(records)
        n = r.nbytes // 144
        G, caps, cap_a, n_a = self._fold_content_args(met, caps)
        kr = np.ascontiguousarray(k8s_rows, dtype=np.uint32)
        nr = np.ascontiguousarray(net_rows, dtype=NET_ROW) if net_rows is not None else None
        feat, keep = (None, None)
        if features is not None and features[0] is not None:
            feat, keep = self._pb_features(n, features[0], {k: v for k, v in self._content_parts(features[1]).items() if v is not None})
        outs = [np.zeros(min(c, L.MET_MAX_GROUPS), dtype=METRIC_GROUP_CONTENT) for c in caps]
        ptrs = (C.c_void_p * G)(*[o.ctypes.data if o.size else None for o in outs])
        rc = L.lib.nfagg_metrics_fold_content(self._h, met._t, r.ctypes.data_as(C.c_void_p) if n else None, n, C.byref(feat) if feat is not None else None,
                                              kr.ctypes.data_as(C.c_void_p) if n else None,
                                              nr.ctypes.data_as(C.c_void_p) if nr is not None and n else None, cap_a, ptrs, n_a)
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        counts = [int(x) for x in n_a]
        return rc, [o[:c if rc == L.OK else 0] for o, c in zip(outs, counts)], counts

    def metrics_fold_content_device(self, met: "MetricsTable", d_records: int, n: int, d_k8s_rows: int, d_net_rows: int, caps, d_outs, d_features=None):
        """Device-resident variant (raw device pointers; d_features = (d_present, {part: pointer}) or None; d_outs[g]: room for
        caps[g] groups of 128 bytes, 16-byte aligned). Returns (rc, n_groups)."""
        G, caps, cap_a, n_a = self._fold_content_args(met, caps)
        ptrs = (C.c_void_p * G)(*[p or None for p in d_outs])
        feat = self._pb_features(n, d_features[0], self._content_parts(d_features[1]), device=True)[0] if d_features is not None else None
        rc = L.lib.nfagg_metrics_fold_content_device(self._h, met._t, C.c_void_p(d_records or None), n, C.byref(feat) if feat is not None else None,
                                                     C.c_void_p(d_k8s_rows or None), C.c_void_p(d_net_rows or None), cap_a, ptrs, n_a)
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        return rc, [int(x) for x in n_a]

    # -- extract timebased (nfagg_timebased_*): the windowed GROUP BY and top-K; timebased.ExtractTimebased is the host side
    def timebased_rules(self, rules, k8s: "K8sTable" = None, net: "NetTable" = None, max_keys: int = 1 << 16) -> "TimebasedRules":
        """The rule set on this handle's device. rules: dicts of index_keys, operation (L.TB_OP_*), value (L.MET_VALUE_* 1..6),
        top_k, reversed, interval_ns (TimebasedRules.rule)."""
        return TimebasedRules(rules, k8s, net, max_keys, self)

    def _tb_outs(self, tb, caps):
        R = len(tb.rules)
        caps = [int(caps)] * R if np.isscalar(caps) else [int(c) for c in caps]
        return R, caps, (C.c_uint32 * R)(*caps), (C.c_uint32 * R)()

    def timebased_extract(self, tb: "TimebasedRules", records: np.ndarray, now_ns: int, k8s_rows: np.ndarray = None, net_rows: np.ndarray = None,
                          features=None, caps=4096):
        """nfagg_timebased_extract. features: (present, parts) or None. caps: one cap, or one per rule. Returns (rc, results,
        n_out, n_missing): results[r] is a TB_RESULT array in the reference's order; with rc == L.TRUNCATED or L.EDEFER every
        results[r] is empty (after L.TRUNCATED the windows HAVE advanced: take the results with timebased_results)."""
        r = np.ascontiguousarray(records)
        n = r.nbytes // 144
        R, caps, cap_a, n_a = self._tb_outs(tb, caps)
        kr = np.ascontiguousarray(k8s_rows, dtype=np.uint32) if k8s_rows is not None else None
        nr = np.ascontiguousarray(net_rows, dtype=NET_ROW) if net_rows is not None else None
        feat, keep = (None, None)
        if features is not None and features[0] is not None:
            feat, keep = self._pb_features(n, features[0], {k: v for k, v in self._content_parts(features[1]).items() if v is not None})
        outs = [np.zeros(min(c, tb.max_keys), dtype=TB_RESULT) for c in caps]
        ptrs = (C.c_void_p * R)(*[o.ctypes.data if o.size else None for o in outs])
        missing = C.c_uint64(0)
        rc = L.lib.nfagg_timebased_extract(self._h, tb._t, r.ctypes.data_as(C.c_void_p) if n else None, n, C.byref(feat) if feat is not None else None,
                                           kr.ctypes.data_as(C.c_void_p) if kr is not None and n else None,
                                           nr.ctypes.data_as(C.c_void_p) if nr is not None and n else None, now_ns, cap_a, ptrs, n_a, C.byref(missing))
        self._check(rc, ok=(L.OK, L.TRUNCATED, L.EDEFER))
        counts = [int(x) for x in n_a]
        return rc, [o[:c if rc == L.OK else 0] for o, c in zip(outs, counts)], counts, int(missing.value)

    def timebased_extract_device(self, tb: "TimebasedRules", d_records: int, n: int, now_ns: int, d_k8s_rows: int, d_net_rows: int, caps, d_outs,
                                 d_features=None):
        """Device-resident variant (raw device pointers; 0: none; d_outs[r]: room for caps[r] results of 16 bytes, 16-byte
        aligned). Returns (rc, n_out, n_missing)."""
        R, caps, cap_a, n_a = self._tb_outs(tb, caps)
        ptrs = (C.c_void_p * R)(*[p or None for p in d_outs])
        feat = self._pb_features(n, d_features[0], self._content_parts(d_features[1]), device=True)[0] if d_features is not None else None
        missing = C.c_uint64(0)
        rc = L.lib.nfagg_timebased_extract_device(self._h, tb._t, C.c_void_p(d_records or None), n, C.byref(feat) if feat is not None else None,
                                                  C.c_void_p(d_k8s_rows or None), C.c_void_p(d_net_rows or None), now_ns, cap_a, ptrs, n_a, C.byref(missing))
        self._check(rc, ok=(L.OK, L.TRUNCATED, L.EDEFER))
        return rc, [int(x) for x in n_a], int(missing.value)

    def timebased_results(self, tb: "TimebasedRules", caps=4096):
        """nfagg_timebased_results: the rules again at the last call's now. Returns (rc, results, n_out)."""
        R, caps, cap_a, n_a = self._tb_outs(tb, caps)
        outs = [np.zeros(min(c, tb.max_keys), dtype=TB_RESULT) for c in caps]
        ptrs = (C.c_void_p * R)(*[o.ctypes.data if o.size else None for o in outs])
        rc = L.lib.nfagg_timebased_results(self._h, tb._t, cap_a, ptrs, n_a)
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        counts = [int(x) for x in n_a]
        return rc, [o[:c if rc == L.OK else 0] for o, c in zip(outs, counts)], counts

    def timebased_results_device(self, tb: "TimebasedRules", caps, d_outs):
        R, caps, cap_a, n_a = self._tb_outs(tb, caps)
        ptrs = (C.c_void_p * R)(*[p or None for p in d_outs])
        rc = L.lib.nfagg_timebased_results_device(self._h, tb._t, cap_a, ptrs, n_a)
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        return rc, [int(x) for x in n_a]

    # -- conversation tracking (nfagg_conn_*): the per-call fold under FLP's `extract conntrack`; conntrack.ConnTrack is the host side
    def conn_fold(self, records: np.ndarray, now_unix_ns: int, mono_now_ns: int, cap: int = 4096, hash_ids: bool = True):
        """nfagg_conn_fold. Returns (rc, partials, n_conns, hash_ids, n_discarded): partials is a CONN_PARTIAL array in unspecified
        order (sort by first_idx); with rc == L.TRUNCATED it is empty and n_conns is a lower bound above cap. hash_ids: uint64
        per record, 0 for a discarded flow, or None when not asked for."""
        r = np.ascontiguousarray(records)
        n = r.nbytes // 144
        opt = L.ConnOptions(struct_size=C.sizeof(L.ConnOptions), now_unix_ns=now_unix_ns, mono_now_ns=mono_now_ns)
        out = np.zeros(min(int(cap), L.CONN_MAX_CONNS), dtype=CONN_PARTIAL)
        ids = np.zeros(n, dtype=np.uint64) if hash_ids else None
        n_conns, n_disc = C.c_uint32(0), C.c_uint32(0)
        rc = L.lib.nfagg_conn_fold(self._h, r.ctypes.data_as(C.c_void_p) if n else None, n, C.byref(opt),
                                   ids.ctypes.data_as(C.c_void_p) if hash_ids and n else None, int(cap),
                                   out.ctypes.data_as(C.c_void_p) if out.size else None, C.byref(n_conns), C.byref(n_disc))
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        return rc, out[:n_conns.value if rc == L.OK else 0], n_conns.value, ids, n_disc.value

    def conn_fold_device(self, d_records: int, n: int, now_unix_ns: int, mono_now_ns: int, d_hash_ids: int, cap: int, d_out: int):
        """Device-resident variant (raw device pointers; d_hash_ids = 0: none; d_out: room for cap partials of 128 bytes, 16-byte
        aligned). Returns (rc, n_conns, n_discarded)."""
        opt = L.ConnOptions(struct_size=C.sizeof(L.ConnOptions), now_unix_ns=now_unix_ns, mono_now_ns=mono_now_ns)
        n_conns, n_disc = C.c_uint32(0), C.c_uint32(0)
        rc = L.lib.nfagg_conn_fold_device(self._h, C.c_void_p(d_records or None), n, C.byref(opt), C.c_void_p(d_hash_ids or None), int(cap),
                                          C.c_void_p(d_out or None), C.byref(n_conns), C.byref(n_disc))
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        return rc, n_conns.value, n_disc.value

    # -- write loki (nfagg_loki_*; loki.py): the stage's table, the plan of one call, its PushRequest bodies
    def loki_table(self, writer, k8s: "K8sTable", net: "NetTable"):
        """A loki.LokiTable on this handle's device; writer: a loki.WriteLoki."""
        from .loki import LokiTable
        return LokiTable(writer, k8s, net, self)

    def loki_plan(self, records: np.ndarray, tls_names: "TlsNames", k8s: "K8sTable", net: "NetTable", loki, now_unix_ns: int, mono_now_ns: int,
                  names: np.ndarray, agent_ip=None, time_received: int = 0, unknown: bytes = b"unknown", hash_ids=None, loki_now_ns: int = None,
                  stream_cap: int = None, group_cap: int = None, present=None, parts=None, rows=None, netev_table: "NetevTable" = None):
        """nfagg_loki_plan: streams, batches and groups of one call's flows (loki.loki_plan); present / parts / rows / netev_table as
        encode_flp_json_conn takes them. Returns (rc, streams, groups,
        deferred, counts); the handle keeps the plan for loki_write."""
        from .loki import loki_plan
        return loki_plan(self, records, tls_names, k8s, net, loki, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown, hash_ids,
                         loki_now_ns, stream_cap, group_cap, present, parts, rows, netev_table)

    def loki_write(self, label_texts, n_batches: int, out_cap: int = None):
        """nfagg_loki_write: the plan's batches as PushRequest bodies, back to back (loki.loki_write). label_texts: every stream's
        LabelSet.String(). Returns (rc, buf, batch_offsets, batch_entries)."""
        from .loki import loki_write
        return loki_write(self, label_texts, n_batches, out_cap)

    # -- write ipfix (nfagg_flp_ipfix_*): FLP's `write ipfix` stage, the enriched flow with the writer's carried element state
    def flp_ipfix_strings(self, entries):
        """A flp_ipfix.IpfixStrings on this handle's device; entries as K8sTable takes them."""
        from .flp_ipfix import IpfixStrings
        return IpfixStrings(entries, self)

    def flp_ipfix_writer(self):
        """A flp_ipfix.IpfixWriterState on this handle's device: the element state of both families."""
        from .flp_ipfix import IpfixWriterState
        return IpfixWriterState(self)

    def flp_ipfix_write(self, state, records: np.ndarray, options, present=None, parts=None, k8s_rows=None, strings=None, out_cap: int = None):
        """nfagg_flp_ipfix_write: one IPFIX message per sent flow (flp_ipfix.flp_ipfix_write). options: flp_ipfix.flp_ipfix_options(...).
        Returns (rc, buf, msg_offsets, status, n_sent)."""
        from .flp_ipfix import flp_ipfix_write
        return flp_ipfix_write(self, state, records, options, present, parts, k8s_rows, strings, out_cap)

    # -- transform filter (nfagg_filter_*): FLP's `transform filter` stage as a device program, the stable compaction, the gather
    def filter(self, spec, k8s: "K8sTable" = None, net: "NetTable" = None) -> "Filter":
        """A compiled filter on this handle's device; spec: a filter.TransformFilter (or anything with its spec())."""
        return Filter(spec, k8s, net, self)

    def filter_apply(self, flt: "Filter", records: np.ndarray, k8s_rows: np.ndarray = None, net_rows: np.ndarray = None, features=None,
                     now_unix_ns: int = 0, mono_now_ns: int = 0, seed: int = 0, first_index: int = 0, cap: int = None, out_records: bool = True):
        """nfagg_filter_apply. features: (present, parts) as encode_flp_json_content takes them, or None. cap: room for the kept
        (default: every flow). Returns (rc, keep uint8[n], rule uint8[n], kept_idx uint32[n_kept], out_records FLOW_RECORD[n_kept] or
        None, n_kept, n_deferred); with rc == L.TRUNCATED kept_idx and out_records are empty and n_kept is exact."""
        r = np.ascontiguousarray(records)
        n = r.nbytes // 144
        cap = n if cap is None else int(cap)
        kr = np.ascontiguousarray(k8s_rows, dtype=np.uint32) if k8s_rows is not None else None
        nr = np.ascontiguousarray(net_rows, dtype=NET_ROW) if net_rows is not None else None
        feat, keep_alive = (None, None)
        if features is not None and features[0] is not None:
            feat, keep_alive = self._pb_features(n, features[0], {k: v for k, v in self._content_parts(features[1]).items() if v is not None})
        keep, rule = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        idx = np.zeros(min(cap, n), dtype=np.uint32)
        out = np.zeros(min(cap, n), dtype=FLOW_RECORD) if out_records else None
        o, _ = flp_options(now_unix_ns, mono_now_ns)
        n_kept, n_def = C.c_size_t(0), C.c_size_t(0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        rc = L.lib.nfagg_filter_apply(self._h, flt._t, ptr(r), n, C.byref(feat) if feat is not None else None, ptr(kr), ptr(nr), C.byref(o),
                                      seed, first_index, ptr(keep), ptr(rule), ptr(idx), ptr(out), cap, C.byref(n_kept), C.byref(n_def))
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        k = n_kept.value if rc == L.OK else 0
        return rc, keep, rule, idx[:k], (out[:k] if out is not None else None), n_kept.value, n_def.value

    def filter_apply_device(self, flt: "Filter", d_records: int, n: int, d_k8s_rows: int = 0, d_net_rows: int = 0, d_features=None,
                            now_unix_ns: int = 0, mono_now_ns: int = 0, seed: int = 0, first_index: int = 0, d_keep: int = 0, d_rule: int = 0,
                            d_kept_idx: int = 0, d_out_records: int = 0, cap: int = 0):
        """Device-resident variant (raw device pointers; d_features = (d_present, {part: pointer}) or None). Returns (rc, n_kept,
        n_deferred)."""
        feat = self._pb_features(n, d_features[0], self._content_parts(d_features[1]), device=True)[0] if d_features is not None else None
        o, _ = flp_options(now_unix_ns, mono_now_ns)
        n_kept, n_def = C.c_size_t(0), C.c_size_t(0)
        rc = L.lib.nfagg_filter_apply_device(self._h, flt._t, C.c_void_p(d_records or None), n, C.byref(feat) if feat is not None else None,
                                             C.c_void_p(d_k8s_rows or None), C.c_void_p(d_net_rows or None), C.byref(o), seed, first_index,
                                             C.c_void_p(d_keep or None), C.c_void_p(d_rule or None), C.c_void_p(d_kept_idx or None),
                                             C.c_void_p(d_out_records or None), cap, C.byref(n_kept), C.byref(n_def))
        self._check(rc, ok=(L.OK, L.TRUNCATED))
        return rc, n_kept.value, n_def.value

    def gather(self, src: np.ndarray, kept_idx: np.ndarray) -> np.ndarray:
        """nfagg_gather: src[kept_idx] along the first axis for a side array that travels with the records (rows, hash ids, present
        bits, parts); an element is 1, 2, 4, 8 or a multiple of 8 up to 64 bytes."""
        a = np.ascontiguousarray(src)
        idx = np.ascontiguousarray(kept_idx, dtype=np.uint32)
        elem = a.nbytes // len(a) if len(a) else (a.dtype.itemsize * int(np.prod(a.shape[1:], dtype=np.int64)))
        out = np.zeros((idx.size,) + a.shape[1:], dtype=a.dtype)
        self._check(L.lib.nfagg_gather(self._h, a.ctypes.data_as(C.c_void_p) if a.size else None, len(a), elem,
                                       idx.ctypes.data_as(C.c_void_p) if idx.size else None, idx.size,
                                       out.ctypes.data_as(C.c_void_p) if idx.size else None))
        return out

    def gather_device(self, d_src: int, n_src: int, elem_bytes: int, d_kept_idx: int, n_kept: int, d_dst: int) -> None:
        """Device-resident variant (raw device pointers)."""
        self._check(L.lib.nfagg_gather_device(self._h, C.c_void_p(d_src or None), n_src, elem_bytes, C.c_void_p(d_kept_idx or None), n_kept,
                                              C.c_void_p(d_dst or None)))

    def stats(self) -> L.Stats:
        s = L.Stats()
        self._check(L.lib.nfagg_stats_get(self._h, C.byref(s)))
        return s

    def reset_profile(self):
        self._check(L.lib.nfagg_stats_reset_profile(self._h))

    def sync(self):
        self._check(L.lib.nfagg_sync(self._h))

    # -- local fold across GPUs, one process per GPU (nfagg_partials_*)
    def set_sequence(self, next_seq: int):
        self._check(L.lib.nfagg_set_sequence(self._h, next_seq))

    @property
    def partial_bytes(self) -> int:
        """nfagg_partial_bytes: 192, or 256 for the sub-flow partials of a kernel-dedup handle."""
        return int(L.lib.nfagg_partial_bytes(self._h))

    def partials_export_device(self, n_shards: int, self_shard: int, d_out: int, cap: int):
        """The live flows as partials of partial_bytes grouped by owner shard, into device memory at d_out (room for cap partials).
        Returns (rc, counts[n_shards], n): rc TRUNCATED = nothing written, n partials needed."""
        counts = (C.c_uint64 * n_shards)()
        n = C.c_size_t(0)
        rc = L.lib.nfagg_partials_export_device(self._h, n_shards, self_shard, C.c_void_p(d_out or None), cap, counts, C.byref(n))
        self._check(rc, (L.OK, L.TRUNCATED))
        return rc, [int(x) for x in counts], n.value

    def partials_merge_device(self, n_shards: int, shard_id: int, d_partials: int, n: int):
        self._check(L.lib.nfagg_partials_merge_device(self._h, n_shards, shard_id, C.c_void_p(d_partials or None), n))

    def window_restart_device(self, n_shards: int, shard_id: int, d_partials: int, n: int, next_seq: int):
        self._check(L.lib.nfagg_window_restart_device(self._h, n_shards, shard_id, C.c_void_p(d_partials or None), n, next_seq))

    def evict_owned_device(self, n_shards: int, shard_id: int, d_out: int, cap: int, reason=L.REASON_TIMEOUT):
        """Returns (rc, n): rc TRUNCATED = nothing evicted, n records needed."""
        n = C.c_size_t(0)
        rc = L.lib.nfagg_evict_owned_device(self._h, reason, n_shards, shard_id, C.c_void_p(d_out or None), cap, C.byref(n))
        self._check(rc, (L.OK, L.TRUNCATED))
        return rc, n.value

    def debug_skip_sequence(self, records: int):
        self._check(L.lib.nfagg_debug_skip_sequence(self._h, records))

    @property
    def stream(self) -> int:
        return L.lib.nfagg_stream(self._h) or 0


class _Member(FlowTable):
    """A group member's handle, borrowed: queries only (sketches, stats, export); the group owns and destroys it."""

    def __init__(self, handle, max_entries):
        self._h = C.c_void_p(handle)
        self.max_entries = max_entries

    def close(self):
        self._h = None


class FlowGroup:
    """nfagg_group (include/nfagg.h): N GPUs behind one process; flows shard by key hash, member i owns shard i.
    local_fold: NFAGG_GROUP_LOCAL_FOLD — chunks are folded where they arrive, the members' slots are merged into their
    owners at the eviction."""

    def __init__(self, devices, max_entries=5000, mode=L.MODE_ACCOUNTER, sketches=0, cm_depth=0, cm_log2_width=0, hll_p=0,
                 staging_records=0, profile=False, ingest_variant=0, local_fold=False):
        cfg = L.Config()
        cfg.struct_size = C.sizeof(L.Config)
        cfg.max_entries = max_entries
        cfg.mode = mode
        cfg.sketch_flags = sketches
        cfg.cm_depth, cfg.cm_log2_width, cfg.hll_p = cm_depth, cm_log2_width, hll_p
        cfg.staging_records = staging_records
        cfg.profile = 1 if profile else 0
        cfg.ingest_variant = ingest_variant
        cfg.group_flags = L.GROUP_LOCAL_FOLD if local_fold else 0
        self.local_fold = bool(local_fold)
        devs = (C.c_int32 * len(devices))(*devices)
        self._g = C.c_void_p()
        rc = L.lib.nfagg_group_create(C.byref(cfg), devs, len(devices), C.byref(self._g))
        if rc != L.OK:
            msg = L.lib.nfagg_group_last_error(None)
            self._g = None
            raise NfaggError(rc, msg.decode() if msg else "nfagg_group_create failed")
        self.n = len(devices)
        self.max_entries = max_entries
        share = max_entries if local_fold else (max_entries + self.n - 1) // self.n
        self.members = [_Member(L.lib.nfagg_group_member(self._g, i), share) for i in range(self.n)]

    def close(self):
        if getattr(self, "_g", None):
            for m in self.members:
                m.close()
            L.lib.nfagg_group_destroy(self._g)
            self._g = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, ok=(L.OK,)):
        if rc not in ok:
            msg = L.lib.nfagg_group_last_error(self._g)
            raise NfaggError(rc, msg.decode() if msg else "")
        return rc

    def ingest(self, records: np.ndarray):
        records = np.ascontiguousarray(records)
        n = records.nbytes // 144
        consumed = C.c_size_t(0)
        rc = L.lib.nfagg_group_ingest(self._g, records.ctypes.data_as(C.c_void_p), n, C.byref(consumed))
        self._check(rc, (L.OK, L.FULL))
        return rc, consumed.value

    def ingest_device(self, src_member: int, d_ptr: int, n: int):
        consumed = C.c_size_t(0)
        rc = L.lib.nfagg_group_ingest_device(self._g, src_member, C.c_void_p(d_ptr), n, C.byref(consumed))
        self._check(rc, (L.OK, L.FULL))
        return rc, consumed.value

    def __len__(self):
        v = C.c_uint64(0)
        self._check(L.lib.nfagg_group_len(self._g, C.byref(v)))
        return v.value

    def merge_sketches(self):
        self._check(L.lib.nfagg_group_merge_sketches(self._g))

    def debug_skip_sequence(self, records: int):
        self._check(L.lib.nfagg_group_debug_skip_sequence(self._g, records))

    def evict(self, reason=L.REASON_TIMEOUT) -> np.ndarray:
        cap = max(len(self), 1)
        out = np.zeros(cap, dtype=FLOW_RECORD)
        n = C.c_size_t(0)
        self._check(L.lib.nfagg_group_evict(self._g, reason, out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[: n.value]

    def evict_device(self, d_ptrs, caps, reason=L.REASON_TIMEOUT):
        """Shard i's flows into device buffer d_ptrs[i] (on member i's device). Returns the per-member counts."""
        p = (C.c_void_p * self.n)(*d_ptrs)
        c = (C.c_size_t * self.n)(*caps)
        n = (C.c_size_t * self.n)()
        rc = L.lib.nfagg_group_evict_device(self._g, reason, p, c, n)
        if rc == L.TRUNCATED:        # nothing was evicted; n holds what every member needs
            raise NfaggError(rc, "device buffers too small, needed %s" % [int(x) for x in n])
        self._check(rc)
        return [int(x) for x in n]


IPFIX_TEMPLATE_ID_V4, IPFIX_TEMPLATE_ID_V6 = 256, 257      # go-ipfix NewTemplateID() from 255: v4 is created first


_CONTENT_PARTS = ("additional", "dns", "drops", "xlat", "quic")     # the parts nfagg_pb_features carries


def _netev_entry(cookie: bytes, event):
    """nfagg_netev_entry of one decoder answer. event: an ACL as (action, actor, name, namespace, direction, string) with
    string = the event's String(); any other event as its String() (bytes or str); None or an exception: the decoder failed."""
    e = L.NetevEntry()
    cookie = bytes(cookie)
    assert len(cookie) == 8
    e.cookie[:] = list(cookie)
    enc = lambda v: v.encode() if isinstance(v, str) else bytes(v)
    if event is None or isinstance(event, BaseException):
        e.kind = L.NETEV_UNDECODABLE
    elif isinstance(event, (bytes, str)):
        e.kind = L.NETEV_OTHER
        e.string, e.string_len = enc(event), len(enc(event))      # not len(e.string): reading a c_char_p back stops at a NUL
    else:
        e.kind = L.NETEV_ACL
        for f, v in zip(("action", "actor", "name", "namespace_", "direction", "string"), event):
            setattr(e, f, enc(v))
        e.action_len, e.actor_len, e.name_len, e.namespace_len, e.direction_len, e.string_len = (len(enc(v)) for v in event)
    return e


def netev_render(event, fmt: int) -> bytes:
    """nfagg_netev_render: the JSON object (L.NETEV_JSON) or the serialized pbflow.NetworkEvent (L.NETEV_PB) of one decoder
    answer (see _netev_entry), as the encoders emit it. Host only."""
    e = _netev_entry(bytes(8), event)
    buf = np.zeros(L.NETEV_MAX_RENDERED, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = L.lib.nfagg_netev_render(C.byref(e), fmt, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n))
    if rc != L.OK:
        raise NfaggError(rc, (L.lib.nfagg_last_error(None) or b"").decode())
    return buf[: n.value].tobytes()


class _CallerTable:
    """What the five caller tables share: the library's table `_t`, the FlowTable it was created for (`_owner`; None: a table
    built and checked on the host only) and the table's life cycle."""

    def _create(self, table, destroy, create):
        """create(h, out) calls the library's create function with the owner's handle (or None) and the place for the table;
        `destroy` is the function that frees it."""
        self._t = C.c_void_p()
        h = table._h if table is not None else None
        rc = create(h, C.byref(self._t))
        if rc != L.OK:
            self._t = None
            raise NfaggError(rc, (L.lib.nfagg_last_error(h) or b"").decode())
        self._owner, self._destroy = table, destroy      # the handle must outlive the table

    def close(self):
        if getattr(self, "_t", None):
            if self._owner is None or self._owner._h:
                self._destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class NetevTable(_CallerTable):
    """The OVN sample decoder's answers as a table (nfagg_netev_table_create): entries = [(cookie8, event)], event as
    _netev_entry takes it. With a FlowTable the table lives on its device and serves netev_resolve and the *_netev encoders;
    with table=None it is built and checked on the host only. Row r, as netev_resolve reports it, is cookies[r]: the cookies
    in ascending order of their little-endian 64-bit value."""

    def __init__(self, entries, table: "FlowTable" = None):
        entries = list(entries)
        arr = (L.NetevEntry * max(len(entries), 1))(*[_netev_entry(c, ev) for c, ev in entries])
        self._create(table, L.lib.nfagg_netev_table_destroy, lambda h, out: L.lib.nfagg_netev_table_create(h, arr, len(entries), out))
        self.cookies = sorted((bytes(c) for c, _ in entries), key=lambda c: int.from_bytes(c, "little"))

    def __len__(self):
        return len(self.cookies)


# Go's crypto/tls names as product data: tls.VersionName of 0x0300..0x0304, tls.CipherSuiteName of CipherSuites() and
# InsecureCipherSuites(), tls.CurveID.String() of the curve constants.
GO_TLS_NAMES = (
    [(L.TLS_VERSION, i, n) for i, n in ((0x0300, "SSLv3"), (0x0301, "TLS 1.0"), (0x0302, "TLS 1.1"), (0x0303, "TLS 1.2"), (0x0304, "TLS 1.3"))] +
    [(L.TLS_CIPHER_SUITE, i, n) for i, n in (
        (0x0005, "TLS_RSA_WITH_RC4_128_SHA"), (0x000a, "TLS_RSA_WITH_3DES_EDE_CBC_SHA"), (0x002f, "TLS_RSA_WITH_AES_128_CBC_SHA"),
        (0x0035, "TLS_RSA_WITH_AES_256_CBC_SHA"), (0x003c, "TLS_RSA_WITH_AES_128_CBC_SHA256"), (0x009c, "TLS_RSA_WITH_AES_128_GCM_SHA256"),
        (0x009d, "TLS_RSA_WITH_AES_256_GCM_SHA384"), (0x1301, "TLS_AES_128_GCM_SHA256"), (0x1302, "TLS_AES_256_GCM_SHA384"),
        (0x1303, "TLS_CHACHA20_POLY1305_SHA256"), (0xc007, "TLS_ECDHE_ECDSA_WITH_RC4_128_SHA"),
        (0xc009, "TLS_ECDHE_ECDSA_WITH_AES_128_CBC_SHA"), (0xc00a, "TLS_ECDHE_ECDSA_WITH_AES_256_CBC_SHA"),
        (0xc011, "TLS_ECDHE_RSA_WITH_RC4_128_SHA"), (0xc012, "TLS_ECDHE_RSA_WITH_3DES_EDE_CBC_SHA"),
        (0xc013, "TLS_ECDHE_RSA_WITH_AES_128_CBC_SHA"), (0xc014, "TLS_ECDHE_RSA_WITH_AES_256_CBC_SHA"),
        (0xc023, "TLS_ECDHE_ECDSA_WITH_AES_128_CBC_SHA256"), (0xc027, "TLS_ECDHE_RSA_WITH_AES_128_CBC_SHA256"),
        (0xc02b, "TLS_ECDHE_ECDSA_WITH_AES_128_GCM_SHA256"), (0xc02c, "TLS_ECDHE_ECDSA_WITH_AES_256_GCM_SHA384"),
        (0xc02f, "TLS_ECDHE_RSA_WITH_AES_128_GCM_SHA256"), (0xc030, "TLS_ECDHE_RSA_WITH_AES_256_GCM_SHA384"),
        (0xcca8, "TLS_ECDHE_RSA_WITH_CHACHA20_POLY1305_SHA256"), (0xcca9, "TLS_ECDHE_ECDSA_WITH_CHACHA20_POLY1305_SHA256"))] +
    [(L.TLS_GROUP, i, n) for i, n in ((23, "CurveP256"), (24, "CurveP384"), (25, "CurveP521"), (29, "X25519"), (4588, "X25519MLKEM768"))])


class TlsNames(_CallerTable):
    """The names of TLS versions, cipher suites and groups as a table (nfagg_tls_names_create): entries = [(kind, id, name)],
    kind one of L.TLS_VERSION / L.TLS_CIPHER_SUITE / L.TLS_GROUP, name str or bytes (plain: nothing a JSON string escapes).
    With a FlowTable the table lives on its device and serves encode_flp_json_tls; with table=None it is built and
    checked on the host only, which is enough for render(). An id without a row prints as 0x%04X (version, cipher suite)
    or CurveID(%d) (group).

    GO_TLS_NAMES, the default of FlowTable.tls_names(), is a restatement of Go's crypto/tls tables kept as product data.
    The reference's own test vectors pin only "TLS 1.2", "TLS 1.3", "TLS_AES_256_GCM_SHA384", "X25519" and the 0x0200
    fall-back; the Go shim should not use the list but build its table from its own crypto/tls, so
    that the names follow the Go release it is built with."""

    def __init__(self, entries=GO_TLS_NAMES, table: "FlowTable" = None):
        entries = [(int(k), int(i), n.encode() if isinstance(n, str) else bytes(n)) for k, i, n in entries]
        for k, i, _ in entries:
            if not (0 <= k <= 0xFFFF and 0 <= i <= 0xFFFF):
                raise ValueError("TLS name entry (%d, %d): kind and id are 16-bit values" % (k, i))
        arr = (L.TlsNameEntry * max(len(entries), 1))()
        for e, (k, i, n) in zip(arr, entries):
            e.kind, e.id, e.name, e.name_len = k, i, n, len(n)        # not len(e.name): reading a c_char_p back stops at a NUL
        self._create(table, L.lib.nfagg_tls_names_destroy, lambda h, out: L.lib.nfagg_tls_names_create(h, arr, len(entries), out))
        self.n = len(entries)

    def __len__(self):
        return self.n

    def render(self, kind: int, id: int, mismatch: bool = False) -> bytes:
        """nfagg_tls_names_render: the unquoted string the encoder emits for this value. Host only."""
        if not 0 <= int(id) <= 0xFFFF:
            raise ValueError("id %d does not fit the record's 16-bit field" % id)
        buf = np.zeros(L.TLS_NAME_MAX + 2, dtype=np.uint8)
        n = C.c_size_t(0)
        rc = L.lib.nfagg_tls_names_render(self._t, kind, int(id), 1 if mismatch else 0, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n))
        if rc != L.OK:
            raise NfaggError(rc, (L.lib.nfagg_last_error(None) or b"").decode())
        return buf[: n.value].tobytes()


def _encode_options(cls, now_unix_ns, mono_now_ns, names, unknown):
    """What the three encoders' option structs share: the clocks, the namer table, the unknown name. Returns (options, the
    names array the options point into: keep it alive for the call)."""
    o = cls()
    o.struct_size = C.sizeof(cls)
    o.now_unix_ns, o.mono_now_ns = now_unix_ns, mono_now_ns
    names = np.ascontiguousarray(names if names is not None else np.zeros(0, dtype=INTF_NAME))
    o.names, o.n_names = (names.ctypes.data if len(names) else None), len(names)
    o.unknown_name, o.unknown_len = unknown, len(unknown)
    return o, names


def ipfix_options(now_unix_ns=0, mono_now_ns=0, names=None, export_time_s=0, seq0=0, unknown=b"unknown", obs_domain_id=1,
                  template_ids=(IPFIX_TEMPLATE_ID_V4, IPFIX_TEMPLATE_ID_V6)):
    """nfagg_ipfix_options; returns (options, the names array the options point into: keep it alive for the call)."""
    o, names = _encode_options(L.IpfixOptions, now_unix_ns, mono_now_ns, names, unknown)
    o.export_time_s, o.seq0, o.obs_domain_id = export_time_s & 0xFFFFFFFF, seq0 & 0xFFFFFFFF, obs_domain_id
    o.template_id_v4, o.template_id_v6 = template_ids
    return o, names


def flp_options(now_unix_ns=0, mono_now_ns=0, names=None, agent_ip=None, time_received=0, unknown=b"unknown"):
    """nfagg_flp_options; returns (options, the names array the options point into: keep it alive for the call).
    agent_ip: 16 bytes, 4 bytes (stored v4-mapped, as net.IP prints both alike) or None (nil)."""
    o, names = _encode_options(L.FlpOptions, now_unix_ns, mono_now_ns, names, unknown)
    if agent_ip is None:
        o.agent_ip_nil = 1
    else:
        ip = bytes(agent_ip)
        if len(ip) == 4:
            ip = bytes(10) + b"\xff\xff" + ip
        if len(ip) != 16:
            raise ValueError("agent_ip: 4 or 16 bytes")
        o.agent_ip = (C.c_uint8 * 16)(*ip)
    o.time_received_s = time_received
    return o, names


def ipfix_template(v6: bool, export_time_s: int, seq: int, obs_domain_id: int = 1,
                   template_ids=(IPFIX_TEMPLATE_ID_V4, IPFIX_TEMPLATE_ID_V6)) -> bytes:
    """nfagg_ipfix_template: the 100-byte template message StartIPFIXExporter sends for the v4 or v6 template, with
    Export Time export_time_s and Sequence Number seq (the data records sent so far)."""
    o, _ = ipfix_options(export_time_s=export_time_s, seq0=seq, obs_domain_id=obs_domain_id, template_ids=template_ids)
    buf = (C.c_uint8 * 128)()
    n = C.c_size_t(0)
    rc = L.lib.nfagg_ipfix_template(C.byref(o), 1 if v6 else 0, buf, len(buf), C.byref(n))
    if rc != L.OK:
        raise NfaggError(rc, "nfagg_ipfix_template")
    return bytes(buf[: n.value])


def key_hash(flow_id_bytes: bytes) -> int:
    buf = (C.c_uint8 * 40).from_buffer_copy(bytes(flow_id_bytes)[:40])
    return L.lib.nfagg_key_hash(buf)


def shard_of(flow_id_bytes: bytes, n_shards: int) -> int:
    buf = (C.c_uint8 * 40).from_buffer_copy(bytes(flow_id_bytes)[:40])
    return L.lib.nfagg_shard_of(buf, n_shards)


K8S_FIELDS = ("namespace", "name", "kind", "owner_name", "owner_kind", "network_name", "host_ip", "host_name", "zone")


def _k8s_ip16(ip) -> bytes:
    """net.IP.To16() of an address given as 16 bytes, 4 bytes or text."""
    if isinstance(ip, str):
        import ipaddress
        ip = ipaddress.ip_address(ip).packed
    ip = bytes(ip)
    if len(ip) == 4:
        ip = bytes(10) + b"\xff\xff" + ip
    if len(ip) != 16:
        raise ValueError("an address has 4 or 16 bytes")
    return ip


def _k8s_entry(ip, info: dict):
    """nfagg_k8s_entry of what IndexLookup(nil, ip) returned: info maps K8S_FIELDS to str or bytes (absent: empty); zone None or
    absent: the label does not exist. Returns (entry, the objects it points into)."""
    e = L.K8sEntry()
    e.ip[:] = _k8s_ip16(ip)
    unknown = set(info) - set(K8S_FIELDS)
    if unknown:
        raise ValueError("unknown Kubernetes fields %r" % sorted(unknown))
    keep = []
    for f in K8S_FIELDS:
        v = info.get(f)
        v = b"" if v is None else v.encode() if isinstance(v, str) else bytes(v)
        keep.append(v)
        setattr(e, "namespace_" if f == "namespace" else f, v)
        setattr(e, f + "_len", len(v))
    e.has_zone = 1 if info.get("zone") is not None else 0
    return e, keep


def _k8s_layer(layer):
    """nfagg_k8s_layer of (infra_prefixes, infra_refs): prefixes [str], refs [(namespace, name)]. Returns (struct, keep)."""
    prefixes, refs = layer
    pre = [p.encode() if isinstance(p, str) else bytes(p) for p in prefixes]
    flat = [x.encode() if isinstance(x, str) else bytes(x) for ref in refs for x in ref]
    if any(b"\0" in x for x in pre + flat):
        raise ValueError("layer strings are NUL-terminated")
    a, b = (C.c_char_p * max(len(pre), 1))(*pre), (C.c_char_p * max(len(flat), 1))(*flat)
    s = L.K8sLayer(C.sizeof(L.K8sLayer), len(pre), a, b, len(flat) // 2, 0)
    return s, (a, b, pre, flat)


def k8s_render(ip, info: dict, side: int) -> bytes:
    """nfagg_k8s_render: the block of keys the encoder writes behind SrcAddr (side 0) or DstAddr (side 1) for this answer,
    with its leading comma. Host only."""
    e, keep = _k8s_entry(ip, info)
    buf = np.zeros(L.K8S_MAX_RENDERED, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = L.lib.nfagg_k8s_render(C.byref(e), side, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n))
    if rc != L.OK:
        raise NfaggError(rc, (L.lib.nfagg_last_error(None) or b"").decode())
    return buf[:n.value].tobytes()


class K8sTable(_CallerTable):
    """The Kubernetes informers' answers as a table (nfagg_k8s_table_create): entries = [(ip, info)], ip as 16 bytes, 4 bytes
    or text, info as _k8s_entry takes it (what IndexLookup(nil, ip) returned, plus the zone fillInK8sZone would pick).
    layer: None (no K8S_FlowLayer key) or (infra_prefixes, infra_refs) of the add_kubernetes_infra rule. With a FlowTable
    the table lives on its device and serves k8s_resolve and encode_flp_json_k8s; with table=None it is built and checked on
    the host only. Row r, as k8s_resolve reports it, is entries[r]. Rebuild the table when the informer caches changed."""

    def __init__(self, entries, layer=None, table: "FlowTable" = None):
        entries = list(entries)
        made = [_k8s_entry(ip, info) for ip, info in entries]
        arr = (L.K8sEntry * max(len(made), 1))(*[e for e, _ in made])
        lay, keep = _k8s_layer(layer) if layer is not None else (None, None)
        self._create(table, L.lib.nfagg_k8s_table_destroy,
                     lambda h, out: L.lib.nfagg_k8s_table_create(h, arr, len(made), C.byref(lay) if lay is not None else None, out))
        self.n, self.has_layer = len(made), layer is not None
        self.entries = entries                    # row r is entries[r]: PromCounters turns a class back into texts

    def __len__(self):
        return self.n


NET_ROW = np.dtype([("src_label", "<u2"), ("dst_label", "<u2"), ("direction", "u1"), ("pad_", "u1", (3,))])      # nfagg_net_row


def net_cidrs(categories):
    """The FLP stage's subnetLabels as the flat lists nfagg_net_rules takes: categories = [(name, [CIDR text])] in configuration
    order. Returns ([(ip16, ones, bits, label)], [name bytes]) in walk order, each CIDR as net.ParseCIDR returns it (the
    address as typed, To16; bits 32 for IPv4 text, 128 for IPv6 text). A category without CIDRs is dropped, as parseSubnets
    drops it. Text the stdlib `ipaddress` module refuses raises ValueError."""
    import ipaddress
    cidrs, labels = [], []
    for name, texts in categories:
        texts = list(texts)
        if not texts:
            continue
        labels.append(name.encode() if isinstance(name, str) else bytes(name))
        for text in texts:
            addr, slash, ones = text.partition("/")
            ip = ipaddress.ip_address(addr)
            if not slash or not ones.isdigit() or int(ones) > ip.max_prefixlen:
                raise ValueError("not a CIDR: %r" % text)
            cidrs.append((_k8s_ip16(ip.packed), int(ones), ip.max_prefixlen, len(labels) - 1))
    return cidrs, labels


def _net_rules(flags, cidrs, labels):
    """nfagg_net_rules of flat lists as net_cidrs returns them. Returns (struct, keep)."""
    ca = (L.NetCidr * max(len(cidrs), 1))()
    for k, (ip, ones, bits, label) in enumerate(cidrs):
        ca[k].ip[:] = _k8s_ip16(ip)
        ca[k].ones, ca[k].bits, ca[k].label = ones, bits, label
    texts = [x.encode() if isinstance(x, str) else bytes(x) for x in labels]
    la = (L.NetLabel * max(len(texts), 1))()
    for k, t in enumerate(texts):
        la[k].text, la[k].len = t, len(t)
    return L.NetRules(C.sizeof(L.NetRules), flags, ca, la, len(cidrs), len(texts)), (ca, la, texts)


class NetTable(_CallerTable):
    """Three rules of the FLP `transform network` stage as a table (nfagg_net_table_create). flags: L.NET_REINTERPRET_DIRECTION |
    L.NET_SUBNET_LABELS | L.NET_DECODE_TCP_FLAGS, each rule on its own. categories: the stage's subnetLabels, [(name, [CIDR
    text])] in configuration order (net_cidrs), or with raw=True the flat (cidrs, labels) lists themselves. With a FlowTable
    the table lives on its device and serves net_resolve and encode_flp_json_net; with table=None it is built and checked on
    the host only. Rebuild it when the stage's configuration is updated."""

    def __init__(self, flags: int = 0, categories=(), table: "FlowTable" = None, raw: bool = False):
        cidrs, labels = categories if raw else net_cidrs(categories)
        rules, keep = _net_rules(flags, list(cidrs), list(labels))
        self._create(table, L.lib.nfagg_net_table_destroy, lambda h, out: L.lib.nfagg_net_table_create(h, C.byref(rules), out))
        self.flags, self.n_cidrs, self.n_labels = flags, rules.n_cidrs, rules.n_labels
        self.labels = list(keep[2])               # label k's text, as nfagg_net_row's indexes name it


def net_render(net: "NetTable", side: int, label: int) -> bytes:
    """nfagg_net_render: the fragment the encoder writes behind SrcPort (side 0) or DstPort (side 1) for label `label` of the
    table, with its leading comma; b"" for an empty label. Host only."""
    buf = np.zeros(L.NET_LABEL_MAX + 32, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = L.lib.nfagg_net_render(net._t, side, label, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n))
    if rc != L.OK:
        raise NfaggError(rc, (L.lib.nfagg_last_error(None) or b"").decode())
    return buf[:n.value].tobytes()


class Filter(_CallerTable):
    """A compiled `transform filter` stage (nfagg_filter_create). spec: a filter.TransformFilter; k8s / net: the tables whose rows
    its TABLE atoms index, which must outlive it. With a FlowTable the program lives on its device and serves filter_apply; with
    table=None (and tables built the same way) the spec is checked on the host only."""

    def __init__(self, spec, k8s: "K8sTable" = None, net: "NetTable" = None, table: "FlowTable" = None):
        s, keep = spec.spec() if hasattr(spec, "spec") else spec
        self._create(table, L.lib.nfagg_filter_destroy,
                     lambda h, out: L.lib.nfagg_filter_create(h, k8s._t if k8s is not None else None, net._t if net is not None else None, C.byref(s), out))
        self._tables = (k8s, net)
        self.steps = list(getattr(spec, "steps", ()))     # (kind, group, value, op_begin, op_count): StageFilter reads a keep step's value


def filter_roll(seed: int, flow_index: int, step: int, value: int) -> bool:
    """nfagg_filter_roll: the device path's roll of step `step` for the flow with running index flow_index. Pure CPU."""
    return bool(L.lib.nfagg_filter_roll(seed & (2**64 - 1), flow_index & (2**64 - 1), step, value))


METRIC_GROUP = np.dtype([("src_class", "<u4"), ("dst_class", "<u4"), ("src_label", "<u2"), ("dst_label", "<u2"), ("direction", "u1"), ("layer", "u1"),
                         ("proto", "u1"), ("is_ip", "u1"), ("flows", "<u8"), ("bytes", "<u8"), ("packets", "<u8"), ("flows_with_bytes", "<u8"),
                         ("flows_with_packets", "<u8"), ("pad_", "<u8")])                                           # nfagg_metric_group
assert METRIC_GROUP.itemsize == 64
METRIC_GROUP_CONTENT = np.dtype([("src_class", "<u4"), ("dst_class", "<u4"), ("src_label", "<u2"), ("dst_label", "<u2"), ("direction", "u1"), ("layer", "u1"),
                                 ("proto", "u1"), ("is_ip", "u1"), ("drop_cause", "<u4"), ("drop_state", "<u2"), ("dns_rcode", "u1"), ("ipsec_status", "u1"),
                                 ("bucket", "u1"), ("pad_", "u1", (7,)), ("flows", "<u8"), ("bytes", "<u8"), ("packets", "<u8"), ("flows_with_bytes", "<u8"),
                                 ("flows_with_packets", "<u8"), ("value_sum", "<u8", (2,)), ("flows_with_value", "<u8", (2,)),
                                 ("pad2_", "<u8", (3,))])                                                                   # nfagg_metric_group_content
assert METRIC_GROUP_CONTENT.itemsize == 128


CONN_PARTIAL = np.dtype([("hash_total", "<u8"), ("first_hash_a", "<u8"), ("first_idx", "<u4"), ("last_idx", "<u4"), ("first_fin_idx", "<u4"),
                         ("flags_or", "<u4"), ("flows", "<u8", (2,)), ("bytes", "<u8", (2,)), ("packets", "<u8", (2,)), ("start_ms_min", "<i8"),
                         ("end_ms_max", "<i8"), ("pad_", "<u8", (4,))])                                              # nfagg_conn_partial
assert CONN_PARTIAL.itemsize == 128 == C.sizeof(L.ConnPartial)
CONN_SNAPSHOT = np.dtype([("src_ip", "u1", (16,)), ("dst_ip", "u1", (16,)), ("src_port", "<u2"), ("dst_port", "<u2"), ("eth_protocol", "<u2"),
                          ("proto", "u1"), ("dscp", "u1"), ("src_mac", "u1", (6,)), ("dst_mac", "u1", (6,)), ("n_dirs", "u1"), ("dirs", "u1", (7,)),
                          ("pad_", "<u4"), ("start_ms", "<i8"), ("end_ms", "<i8")])                                  # nfagg_conn_snapshot
CONN_VALUES = np.dtype([("hash_total", "<u8"), ("record_type", "u1"), ("is_first", "u1"), ("pad_", "u1", (6,)), ("flows", "<u8", (2,)),
                        ("bytes", "<u8", (2,)), ("packets", "<u8", (2,)), ("start_ms_min", "<i8"), ("end_ms_max", "<i8"), ("first", CONN_SNAPSHOT),
                        ("last", CONN_SNAPSHOT), ("pad2_", "<u8", (2,))])                                            # nfagg_conn_values
assert CONN_SNAPSHOT.itemsize == 80 and CONN_VALUES.itemsize == 256 and C.sizeof(L.ConnField) == 16


class ConnLayout(_CallerTable):
    """extract conntrack's outputFields compiled into the sorted column program of a conversation line (nfagg_conn_layout_create).
    fields: [dict(name=.., operation=.., input=.., splitAB=..)] as the stage's configuration has them (input defaults to the name;
    count takes none). With a FlowTable the layout lives on its device and serves encode_conn_json; with table=None it is built and
    checked on the host only."""

    def __init__(self, fields, table: "FlowTable" = None):
        arr = (L.ConnField * max(len(fields), 1))()
        keep = []
        for k, f in enumerate(fields):
            name = f.get("name", "")
            name = name.encode("latin-1") if isinstance(name, str) else bytes(name)
            op = f.get("operation", "")
            inp = "" if op == "count" else (f.get("input", "") or f.get("name", ""))
            inp = inp.decode("latin-1") if isinstance(inp, bytes) else inp
            keep.append(name)
            arr[k].name, arr[k].name_len = name, len(name)
            arr[k].op, arr[k].input = L.CONN_OPS.get(op, 255), L.CONN_INPUTS.get(inp, 255)
            arr[k].split_ab = 1 if f.get("splitAB", False) else 0
        self._create(table, L.lib.nfagg_conn_layout_destroy, lambda h, out: L.lib.nfagg_conn_layout_create(h, arr, len(fields), out))
        self.n_columns, self.max_line = L.lib.nfagg_conn_layout_columns(self._t), L.lib.nfagg_conn_layout_max_line(self._t)

    def render(self, column: int) -> bytes:
        """Column `column`'s key fragment (,"name":) in sorted order; b"" for a block."""
        buf, n = np.zeros(8 + 6 * 80, dtype=np.uint8), C.c_size_t(0)
        rc = L.lib.nfagg_conn_layout_render(self._t, column, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n))
        if rc != L.OK:
            raise NfaggError(rc, (L.lib.nfagg_last_error(None) or b"").decode())
        return buf[:n.value].tobytes()


def conn_hash(record) -> tuple:
    """nfagg_conn_hash of one 144-byte record: (hashTotal, hashA, hashB); (0, 0, 0) for a record the conntrack filter discards."""
    buf = (C.c_uint8 * 144).from_buffer_copy(bytes(record)[:144])
    a, b = C.c_uint64(0), C.c_uint64(0)
    return L.lib.nfagg_conn_hash(buf, C.byref(a), C.byref(b)), a.value, b.value


class MetricsTable(_CallerTable):
    """The groupings of the `encode prom` counters over a Kubernetes table (nfagg_metrics_table_create). groupings: up to
    L.MET_MAX_GROUPINGS masks of L.DIM_SRC_K8S(f) / L.DIM_DST_K8S(f) (f: index into K8S_FIELDS), L.DIM_SRC_SUBNET_LABEL,
    L.DIM_DST_SUBNET_LABEL, L.DIM_FLOW_DIRECTION, L.DIM_FLOW_LAYER, L.DIM_PROTO. Every row of `k8s` gets a class per grouping
    and side: the dense id, from 1, of the tuple of its selected fields; class_row turns a class back into a row of the
    caller's entries. With a FlowTable (the one `k8s` lives on) the table serves metrics_fold; with table=None (and a host-only
    `k8s`) it is built and checked on the host alone. Rebuild it when the Kubernetes table is rebuilt.

    With specs (nfagg_metrics_table_create_specs; `groupings` is then ignored) every grouping is a dict as spec() takes it:
    dims, xdims (L.XDIM_*), value (up to two L.MET_VALUE_*), hist (0, or 1 / 2: the value slot to bucket) and bounds (integer
    thresholds that do not decrease). Such a table serves metrics_fold_content only."""

    @staticmethod
    def spec(dims=0, xdims=0, value=(), hist=0, bounds=(), struct_size=None, n_bounds=None) -> "L.MetricSpec":
        sp = L.MetricSpec()
        sp.struct_size = C.sizeof(L.MetricSpec) if struct_size is None else struct_size
        sp.dims, sp.xdims, sp.hist = dims & 0xFFFFFFFF, xdims & 0xFFFFFFFF, hist
        for k, v in enumerate(list(value)[:2]):
            sp.value[k] = v
        sp.n_bounds = len(bounds) if n_bounds is None else n_bounds
        for k, b in enumerate(list(bounds)[: L.MET_MAX_BOUNDS]):
            sp.bounds[k] = b
        return sp

    def __init__(self, k8s: "K8sTable", groupings, table: "FlowTable" = None, specs=None):
        if specs is not None:
            self.specs = [sp if isinstance(sp, L.MetricSpec) else self.spec(**sp) for sp in specs]
            self.groupings = [int(sp.dims) for sp in self.specs]
            arr = (L.MetricSpec * max(len(self.specs), 1))(*self.specs)
            self._create(table, L.lib.nfagg_metrics_table_destroy, lambda h, out: L.lib.nfagg_metrics_table_create_specs(h, k8s._t, arr, len(self.specs), out))
        else:
            self.specs = None
            self.groupings = [int(g) for g in groupings]
            arr = (C.c_uint32 * max(len(self.groupings), 1))(*[g & 0xFFFFFFFF for g in self.groupings])
            self._create(table, L.lib.nfagg_metrics_table_destroy, lambda h, out: L.lib.nfagg_metrics_table_create(h, k8s._t, arr, len(self.groupings), out))
        self.k8s = k8s                            # the Kubernetes table must outlive this one, as the handle must

    def n_classes(self, g: int, side: int) -> int:
        return L.lib.nfagg_metrics_n_classes(self._t, g, side)

    def class_row(self, g: int, side: int, cls: int) -> int:
        """The first entry index of class `cls` (L.K8S_NO_ROW for class 0)."""
        row = C.c_uint32(0)
        rc = L.lib.nfagg_metrics_class_row(self._t, g, side, cls, C.byref(row))
        if rc != L.OK:
            raise NfaggError(rc, (L.lib.nfagg_last_error(self._owner._h if self._owner is not None else None) or b"").decode())
        return row.value


TB_RESULT = np.dtype([("key", "<u4"), ("flags", "<u4"), ("value", "<f8")])      # nfagg_tb_result
TB_KEY = np.dtype([("col", "u1", (4, 16))])                                       # nfagg_tb_key


class TimebasedRules(_CallerTable):
    """The rules of `extract timebased` and their tables (nfagg_timebased_rules_create). rules: dicts as rule() takes them, or
    L.TbRule. With a FlowTable the tables live on its device; with table=None the rules are built and checked on the host alone
    (and `k8s` / `net` must be host-only too). The Kubernetes and the net table must outlive the object."""

    @staticmethod
    def rule(index_keys=(), operation=L.TB_OP_SUM, value=L.MET_VALUE_BYTES, top_k=0, reversed=False, interval_ns=0, struct_size=None,
             n_index_keys=None) -> "L.TbRule":
        ru = L.TbRule()
        ru.struct_size = C.sizeof(L.TbRule) if struct_size is None else struct_size
        keys = [k.encode() if isinstance(k, str) else bytes(k) for k in index_keys]
        ru.n_index_keys = len(keys) if n_index_keys is None else n_index_keys
        for k, name in enumerate(keys[: L.TB_MAX_COLUMNS]):
            ru.index_keys[k] = name
        ru.operation, ru.value, ru.top_k, ru.reversed, ru.interval_ns = operation, value, top_k, 1 if reversed else 0, interval_ns
        return ru

    def __init__(self, rules, k8s: "K8sTable" = None, net: "NetTable" = None, max_keys: int = 1 << 16, table: "FlowTable" = None, options=None):
        self.rules = [ru if isinstance(ru, L.TbRule) else self.rule(**ru) for ru in rules]
        arr = (L.TbRule * max(len(self.rules), 1))(*self.rules)
        if options is None:
            options = L.TbOptions(C.sizeof(L.TbOptions), max_keys)
        self.max_keys = int(options.max_keys)
        self._create(table, L.lib.nfagg_timebased_destroy,
                     lambda h, out: L.lib.nfagg_timebased_rules_create(h, k8s._t if k8s is not None else None, net._t if net is not None else None, arr,
                                                                       len(self.rules), C.byref(options), out))
        self.k8s, self.net = k8s, net
        st = self.stats()
        self.table_of_rule = [int(st.table_of_rule[r]) for r in range(len(self.rules))]

    def _err(self, rc):
        return NfaggError(rc, (L.lib.nfagg_last_error(self._owner._h if self._owner is not None else None) or b"").decode())

    def stats(self) -> "L.TbStats":
        st = L.TbStats()
        rc = L.lib.nfagg_timebased_stats(self._t, C.byref(st))
        if rc != L.OK:
            raise self._err(rc)
        return st

    def reset(self) -> None:
        rc = L.lib.nfagg_timebased_reset(self._t)
        if rc != L.OK:
            raise self._err(rc)

    def keys(self, table: int, ids) -> np.ndarray:
        """nfagg_timebased_keys: the columns of the keys `ids` of table `table`, a TB_KEY array."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.zeros(len(ids), dtype=TB_KEY)
        rc = L.lib.nfagg_timebased_keys(self._t, table, ids.ctypes.data_as(C.c_void_p), len(ids), out.ctypes.data_as(C.c_void_p))
        if rc != L.OK:
            raise self._err(rc)
        return out

    def class_row(self, table: int, column: int, cls: int) -> int:
        row = C.c_uint32(0)
        rc = L.lib.nfagg_timebased_class_row(self._t, table, column, cls, C.byref(row))
        if rc != L.OK:
            raise self._err(rc)
        return row.value

    def key_hash(self, table: int, keys) -> np.ndarray:
        """nfagg_timebased_key_hash of every TB_KEY of `keys`."""
        keys = np.ascontiguousarray(np.atleast_1d(keys), dtype=TB_KEY)
        base = keys.ctypes.data
        return np.array([L.lib.nfagg_timebased_key_hash(self._t, table, C.c_void_p(base + 64 * k)) for k in range(len(keys))], dtype=np.uint64)


def ip_hash(ip16: bytes, seed_index: int) -> int:
    buf = (C.c_uint8 * 16).from_buffer_copy(bytes(ip16))
    return L.lib.nfagg_ip_hash(buf, seed_index)


def metrics_group_hash(grouping: int, groups) -> np.ndarray:
    """nfagg_metrics_group_hash of every METRIC_GROUP in `groups` (only the key fields are read) for grouping index `grouping`:
    the hash whose low bits are the group's home slot in the fold's tables. Pure CPU."""
    g = np.ascontiguousarray(np.atleast_1d(groups), dtype=METRIC_GROUP)
    base = g.ctypes.data
    return np.fromiter((L.lib.nfagg_metrics_group_hash(grouping, base + METRIC_GROUP.itemsize * i) for i in range(len(g))), dtype=np.uint64, count=len(g))


def metrics_group_hash_content(grouping: int, groups) -> np.ndarray:
    """nfagg_metrics_group_hash_content of every METRIC_GROUP_CONTENT in `groups` (the thirteen key fields are read). Pure CPU."""
    g = np.ascontiguousarray(np.atleast_1d(groups), dtype=METRIC_GROUP_CONTENT)
    base = g.ctypes.data
    return np.fromiter((L.lib.nfagg_metrics_group_hash_content(grouping, base + METRIC_GROUP_CONTENT.itemsize * i) for i in range(len(g))), dtype=np.uint64,
                       count=len(g))


def flp_enum_name(kind: int, raw: int) -> bytes:
    """nfagg_flp_enum_name: the text the direct-FLP JSON encoders print for a raw DNS response code (L.FLP_ENUM_DNS_RCODE), TCP
    state (L.FLP_ENUM_TCP_STATE) or drop cause (L.FLP_ENUM_DROP_CAUSE). Pure CPU."""
    buf, n = C.create_string_buffer(64), C.c_size_t(0)
    rc = L.lib.nfagg_flp_enum_name(kind, raw & 0xFFFFFFFF, buf, 64, C.byref(n))
    if rc != L.OK:
        raise NfaggError(rc, (L.lib.nfagg_last_error(None) or b"").decode())
    return buf.raw[: n.value]


def hll_estimate_from_histogram(hist, p: int) -> float:
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    assert h.size == 65
    return L.lib.nfagg_hll_estimate_from_histogram(h.ctypes.data_as(C.c_void_p), p)


def record_times(now_unix_ns: int, mono_now_ns: int, metrics: np.void):
    """pkg/model/record.go:90-97 via the library helper."""
    m = np.ascontiguousarray(np.array([metrics], dtype=FLOW_METRICS))
    a, b = C.c_int64(0), C.c_int64(0)
    L.lib.nfagg_record_times(now_unix_ns, mono_now_ns, m.ctypes.data_as(C.c_void_p), C.byref(a), C.byref(b))
    return a.value, b.value
