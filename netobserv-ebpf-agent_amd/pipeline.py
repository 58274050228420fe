"""Host-side mirrors of the two pipeline nodes that sit right after the Accounter, for
BASELINE configs[0] ("10k flow_record_t, 1k 5-tuples, Accounter via direct-flp stdout"):

  CapacityLimiter.Limit(in, out)      pkg/flow/limiter.go:28-38 (drop when the destination buffer is full)
  RecordToMap(record)                 pkg/decode/decode_protobuf.go:63-127, the keys a BpfFlowMetrics-only
                                      record (what the Accounter evicts) produces
  DirectFLPStdout.ExportFlows(in)     pkg/exporter/direct_flp.go + flowlogs-pipeline write_stdout.go:37-51
                                      with `format: json` (one JSON object per flow, keys sorted)
  IPFIX / StartIPFIXExporter          pkg/exporter/ipfix.go over the GPU encoder (nfagg_encode_ipfix)
  DirectFLPJSON / StartDirectFLPJSON  DirectFLPStdout's lines from the GPU encoder (nfagg_encode_flp_json)

Plumbing only — no flow state is touched here; the records come from libnfagg (accounter.py). The
string tables of the feature branch (TCP states, drop causes, DNS rcodes, TLS names) stay with the Go
decoder: RecordToMap refuses records that would need them instead of guessing. (The GPU encoders take the TLS
names as a caller-built table, TlsNames: DirectFLPJSON and MapTracer.evictFlowsJSON with tls_names.)"""
import ipaddress
import json
import queue
import sys
import time
from typing import Callable

import numpy as np

from .accounter import CLOSE, Record
from .records import INTF_NAME
from .table import IPFIX_TEMPLATE_ID_V4, IPFIX_TEMPLATE_ID_V6, ipfix_template


class CapacityLimiter:                                    # limiter.go:19-26
    def __init__(self, metrics=None):
        self.droppedFlows = 0
        self.metrics = metrics

    def Limit(self, inp: "queue.Queue", out: "queue.Queue"):
        """limiter.go:28-38. `out.maxsize` is cap(out); 0 = unbuffered, which never drops."""
        while True:
            batch = inp.get()
            if batch is CLOSE:
                out.put(CLOSE)
                return
            if out.maxsize == 0 or out.qsize() < out.maxsize:
                out.put(batch)
            else:
                if self.metrics is not None:
                    k = ("limiter", "full")
                    self.metrics.dropped_flows_total = getattr(self.metrics, "dropped_flows_total", {})
                    self.metrics.dropped_flows_total[k] = self.metrics.dropped_flows_total.get(k, 0) + len(batch)
                self.droppedFlows += len(batch)


def limit_batches(epoch_end, queue_len: int, queue_cap: int):
    """nfagg_limit_batches: CapacityLimiter.Limit's decision (limiter.go:28-38) for the evictions one nfagg_account call
    delivered, taken before any Record is built. Returns (keep flags, dropped flows)."""
    import ctypes as C
    import numpy as np
    from . import _lib as L
    ends = (C.c_uint64 * max(len(epoch_end), 1))(*[int(x) for x in epoch_end])
    keep = np.zeros(max(len(epoch_end), 1), dtype=np.uint8)
    dropped = C.c_uint64(0)
    L.lib.nfagg_limit_batches(ends, len(epoch_end), queue_len, queue_cap, keep.ctypes.data_as(C.c_void_p), C.byref(dropped))
    return [bool(k) for k in keep[: len(epoch_end)]], dropped.value


def _mac(b) -> str:                                       # net.HardwareAddr.String()
    return ":".join("%02x" % x for x in bytes(b))


def _ip(b) -> str:                                        # model.IP(...).String(): net.IP of 16 bytes
    a = ipaddress.IPv6Address(bytes(b))
    return str(a.ipv4_mapped) if a.ipv4_mapped is not None else str(a)


def _unix_milli(ns: int) -> int:                          # time.Time.UnixMilli(): floor division
    return ns // 1_000_000


def RecordToMap(fr: Record, time_received: int = None) -> dict:
    """decode_protobuf.go:63-127 for a record that carries only BpfFlowMetrics."""
    m, k = fr.Metrics, fr.ID
    if int(m["ssl_version"]) or int(m["tls_types"]) or int(m["tls_cipher_suite"]) or int(m["tls_key_share"]):
        raise NotImplementedError("TLS name tables (crypto/tls) stay with the Go decoder")
    if fr.DNSMetrics is not None or fr.AdditionalMetrics is not None:
        raise NotImplementedError("feature keys stay with the Go decoder")
    out = {
        "SrcMac": _mac(m["src_mac"]), "DstMac": _mac(m["dst_mac"]), "Etype": int(m["eth_protocol"]),
        "TimeFlowStartMs": _unix_milli(fr.TimeFlowStart), "TimeFlowEndMs": _unix_milli(fr.TimeFlowEnd),
        "TimeReceived": int(time.time()) if time_received is None else time_received,
        "AgentIP": str(fr.AgentIP) if fr.AgentIP is not None else "<nil>",
        "IfDirections": [i.Direction for i in fr.Interfaces], "Interfaces": [i.Interface for i in fr.Interfaces],
    }
    if fr.Interfaces:
        out["Udns"] = [i.Udn for i in fr.Interfaces]
    if int(m["bytes"]):
        out["Bytes"] = int(m["bytes"])
    if int(m["packets"]):
        out["Packets"] = int(m["packets"])
    if int(m["sampling"]):
        out["Sampling"] = int(m["sampling"])
    if int(m["eth_protocol"]) in (0x0800, 0x86DD):
        out["SrcAddr"], out["DstAddr"] = _ip(k["src_ip"]), _ip(k["dst_ip"])
        proto = int(k["transport_protocol"])
        out["Proto"], out["Dscp"] = proto, int(m["dscp"])
        if proto in (1, 58):                              # IPPROTO_ICMP, IPPROTO_ICMPV6
            out["IcmpType"], out["IcmpCode"] = int(k["icmp_type"]), int(k["icmp_code"])
        elif proto in (6, 17, 132):                       # TCP, UDP, SCTP
            out["SrcPort"], out["DstPort"] = int(k["src_port"]), int(k["dst_port"])
            if proto == 6:
                out["Flags"] = int(m["flags"])
    if fr.TimeFlowRtt:
        out["TimeFlowRttNs"] = fr.TimeFlowRtt
    return out


class DirectFLPStdout:
    """StartDirectFLP with a lone `write: stdout, format: json` stage (direct_flp_test.go:17-33)."""

    def __init__(self, stream=None, time_received=None):
        self.stream = stream or sys.stdout
        self.time_received = time_received

    def ExportFlows(self, inp: "queue.Queue"):
        while True:
            batch = inp.get()
            if batch is CLOSE:
                return
            for rec in batch:
                self.stream.write(json.dumps(RecordToMap(rec, self.time_received), sort_keys=True, separators=(",", ":")) + "\n")


# ---------------------------------------------------------------------------------------------
# The kernel-map branch: MapTracer (pkg/flow/tracer_map.go:22-146) over a fetcher whose
# LookupAndDeleteMap runs on the GPU (nfagg_map_merge). The eBPF syscalls that drain the maps stay
# with the caller (`drain`); the join, the per-CPU folds and buildBaseFromAdditional are libnfagg's.
from dataclasses import dataclass  # noqa: E402
from typing import Callable, Optional  # noqa: E402

import numpy as np  # noqa: E402

from . import _lib as _L  # noqa: E402
from .accounter import NewRecord  # noqa: E402


@dataclass
class BpfFlowContent:                                     # pkg/model/flow_content.go:9-17 (nil = None)
    BpfFlowMetrics: np.void
    DNSMetrics: Optional[np.void] = None
    PktDropMetrics: Optional[np.void] = None
    NetworkEventsMetrics: Optional[np.void] = None
    XlatMetrics: Optional[np.void] = None
    AdditionalMetrics: Optional[np.void] = None
    QuicMetrics: Optional[np.void] = None


class GPUMapFetcher:
    """mapFetcher (tracer_map.go:37-40) whose LookupAndDeleteMap (pkg/tracer/tracer.go:1022-1116) is one
    nfagg_map_merge call. drain() -> (main_ids, main_vals, {kind: (ids, partials[n, n_cpu])}, n_cpu)."""

    _PARTS = (("dns", "DNSMetrics", _L.FEAT_DNS), ("drops", "PktDropMetrics", _L.FEAT_DROPS),
              ("network_events", "NetworkEventsMetrics", _L.FEAT_NETWORK_EVENTS), ("xlat", "XlatMetrics", _L.FEAT_XLAT),
              ("additional", "AdditionalMetrics", _L.FEAT_ADDITIONAL), ("quic", "QuicMetrics", _L.FEAT_QUIC))

    def __init__(self, table, drain: Callable):
        self.table, self.drain = table, drain

    def LookupAndDeleteMap(self, metrics=None):
        main_ids, main_vals, feats, n_cpu = self.drain()
        recs, present, parts, _dups = self.table.map_merge(main_ids, main_vals, feats, n_cpu)
        flows = []
        for i in range(len(recs)):
            c = BpfFlowContent(BpfFlowMetrics=recs[i]["metrics"])
            for kind, attr, bit in self._PARTS:
                if present[i] & bit:
                    setattr(c, attr, parts[kind][i])
            flows.append((recs[i]["id"], c))
        if metrics is not None:
            metrics.buffer_size["merged-maps"] = len(flows)            # tracer.go:1112
        return flows

    def DeleteMapsStaleEntries(self, timeout):                          # kernel-side housekeeping: stays in Go
        pass


class MapTracer:
    """tracer_map.go:22-60. TraceLoop's ticker / condition variable (:62-101) is goroutine plumbing: callers
    invoke evictFlows directly (what Flush() ends up doing)."""

    def __init__(self, fetcher, eviction_timeout, stale_entries_evict_timeout, metrics=None, s=None, udn_enabled=False,
                 clock=None, mono_clock=None, sample_decoder: Callable = None):
        self.mapFetcher, self.evictionTimeout, self.staleEntriesEvictTimeout = fetcher, eviction_timeout, stale_entries_evict_timeout
        self.metrics, self.s, self.udnEnabled = metrics, s, udn_enabled
        self.clock = clock or (lambda: time.time_ns())
        self.monoClock = mono_clock or (lambda: time.monotonic_ns())
        # model.SampleDecoder as a callable: cookie (8 bytes) -> an ACL as (action, actor, name, namespace, direction, String()),
        # any other event as its String(), or None / a raised exception when DecodeCookie8Bytes fails. Its answers are kept
        # for the tracer's lifetime, and with them the device table they were rendered into: the decoder is asked once per cookie.
        self.sampleDecoder = sample_decoder
        self.decoderCalls = 0
        self._netevAnswers, self._netevTable = {}, None

    def resolveNetworkEvents(self, present, parts, missing_cap: int = 4096):
        """record.go:126-157 for merged flows (map_merge's present / parts) on the GPU: resolve, ask the decoder about the
        cookies the table does not know, rebuild the table, resolve again until nothing is missing. Returns (present_out,
        parts with the decorated drops, rows, table) for encode_flp_json_netev / encode_pb_netev."""
        table = self.mapFetcher.table
        while True:
            if self._netevTable is None:
                self._netevTable = table.netev_table(self._netevAnswers.items())
            p_out, d_out, rows, missing, _ = table.netev_resolve(self._netevTable, present, parts.get("network_events"),
                                                                 parts.get("drops"), missing_cap)
            if not missing:
                return p_out, {**parts, "drops": d_out}, rows, self._netevTable
            for cookie in missing:
                self.decoderCalls += 1
                try:
                    self._netevAnswers[cookie] = self.sampleDecoder(cookie)
                except Exception as e:                                  # err != nil: the cookie's events are skipped
                    self._netevAnswers[cookie] = e
            self._netevTable.close()
            self._netevTable = None

    def evictFlowsJSON(self, names=None, agent_ip=None, time_received: int = 0, unknown: bytes = b"unknown", tls_names=None, k8s=None, net=None,
                       metrics=None, filter=None, loki=None, ipfix=None):
        """evictFlows for a direct-FLP `write: stdout, format: json` stage, without a Record per flow: the drained maps are merged,
        decorated with the sample decoder's network events and encoded on the GPU. Returns (buf, line_offsets, deferred) as
        FlowTable.encode_flp_json_content does; with tls_names (a TlsNames of the fetcher's table) the TLS keys are written too,
        nothing is deferred and the result is (buf, line_offsets) as FlowTable.encode_flp_json_tls gives it. With k8s (a K8sTable of the
        fetcher's table; needs tls_names) the lines carry what the `transform network` stage's Kubernetes rules add as well
        (FlowTable.encode_flp_json_k8s). With net (a NetTable; needs k8s) also what its reinterpret_direction, add_subnet_label and
        decode_tcp_flags rules add (FlowTable.encode_flp_json_net). With metrics (a PromCounters or a PromMetrics; needs k8s) the
        `encode prom` metrics observe the same flows; a PromMetrics is handed the flows' feature parts as well, with a sample
        decoder those nfagg_netev_resolve wrote, so that an injected drop counts like any other. With filter (a filter.StageFilter;
        needs tls_names) the `transform filter` stage runs on the merged flows first: the metrics and the lines are those of the kept
        flows, a third result lists the lines the caller formats itself (their stored Sampling overflows 32 bits) as (position, the
        admitting keep step, the Sampling the reference stores), as StageFilter.apply returns them. With loki (a loki.LokiWriter over
        the same tables; needs net) the pipeline ends in `write loki`: the result is (bodies, deferred, held), the PushRequest bodies
        of the merged (and kept) flows with their feature parts and network events, the positions the caller formats itself because
        of their timestamp, and the filter's held flows as above (with their stored Sampling), which are in no body. With ipfix (a
        flp_ipfix.WriteIpfix of the fetcher's table) the pipeline ends in `write ipfix`: the merged (and kept) flows with their xlat and
        RTT parts, and with k8s their Kubernetes strings (the writer's IpfixStrings over the same entries), go to the writer's send;
        the result is (sent, failed, held), failed as [(position, status)]."""
        if filter is not None and tls_names is None:
            raise ValueError("filter needs tls_names")
        if loki is not None and net is None:
            raise ValueError("loki needs tls_names, k8s and net: the stage's labels are keys of the transform network stage")
        if k8s is not None and tls_names is None:
            raise ValueError("k8s needs tls_names: the enriched encoder defers nothing")
        if net is not None and k8s is None:
            raise ValueError("net needs k8s: reinterpret_direction reads the Kubernetes keys")
        if metrics is not None and k8s is None:
            raise ValueError("metrics needs k8s: the counters group by the Kubernetes keys")
        monotonic_now, current = self.monoClock(), self.clock()
        table = self.mapFetcher.table
        main_ids, main_vals, feats, n_cpu = self.mapFetcher.drain()
        recs, present, parts, _dups = table.map_merge(main_ids, main_vals, feats, n_cpu)
        names = names if names is not None else np.zeros(0, dtype=INTF_NAME)
        mono = monotonic_now & ((1 << 64) - 1)
        content = hasattr(metrics, "histograms")                        # a PromMetrics reads the feature parts
        if filter is not None:
            rows = tab = None
            if self.sampleDecoder is not None:
                present, parts, rows, tab = self.resolveNetworkEvents(present, parts)
            recs, present, parts, rows, held = filter.apply(table, recs, k8s, net, agent_ip, current, mono, present, parts, rows)
            if metrics is not None:
                metrics.observe(table, recs, k8s, net, agent_ip, **(dict(features=(present, parts)) if content else {}))
            args = (current, mono, names, agent_ip, time_received, unknown, present, parts, rows, tab)
            if loki is not None:
                return self._loki(loki, recs, current, mono, time_received, present, parts, rows, tab, held)
            if ipfix is not None:
                return self._ipfix(ipfix, table, k8s, recs, current, mono, present, parts, held)
            if net is not None:
                return table.encode_flp_json_net(recs, tls_names, k8s, net, *args) + (held,)
            if k8s is not None:
                return table.encode_flp_json_k8s(recs, tls_names, k8s, *args) + (held,)
            return table.encode_flp_json_tls(recs, tls_names, *args) + (held,)
        if metrics is not None and not content:
            metrics.observe(table, recs, k8s, net, agent_ip)
        if self.sampleDecoder is None:                                  # s == nil: no events, no injected drops (record.go:126)
            if content:
                metrics.observe(table, recs, k8s, net, agent_ip, features=(present, parts))
            if loki is not None:
                return self._loki(loki, recs, current, mono, time_received, present, parts, None, None, [])
            if ipfix is not None:
                return self._ipfix(ipfix, table, k8s, recs, current, mono, present, parts, [])
            if net is not None:
                return table.encode_flp_json_net(recs, tls_names, k8s, net, current, mono, names, agent_ip, time_received, unknown, present, parts)
            if k8s is not None:
                return table.encode_flp_json_k8s(recs, tls_names, k8s, current, mono, names, agent_ip, time_received, unknown, present, parts)
            if tls_names is not None:
                return table.encode_flp_json_tls(recs, tls_names, current, mono, names, agent_ip, time_received, unknown, present, parts)
            return table.encode_flp_json_content(recs, present, parts, current, mono, names, agent_ip, time_received, unknown)
        p_out, parts, rows, tab = self.resolveNetworkEvents(present, parts)
        if content:
            metrics.observe(table, recs, k8s, net, agent_ip, features=(p_out, parts))
        if loki is not None:
            return self._loki(loki, recs, current, mono, time_received, p_out, parts, rows, tab, [])
        if ipfix is not None:
            return self._ipfix(ipfix, table, k8s, recs, current, mono, p_out, parts, [])
        if net is not None:
            return table.encode_flp_json_net(recs, tls_names, k8s, net, current, mono, names, agent_ip, time_received, unknown, p_out, parts, rows, tab)
        if k8s is not None:
            return table.encode_flp_json_k8s(recs, tls_names, k8s, current, mono, names, agent_ip, time_received, unknown, p_out, parts, rows, tab)
        if tls_names is not None:
            return table.encode_flp_json_tls(recs, tls_names, current, mono, names, agent_ip, time_received, unknown, p_out, parts, rows, tab)
        return table.encode_flp_json_netev(recs, p_out, parts, rows, tab, current, mono, names, agent_ip, time_received, unknown)

    @staticmethod
    def _loki(loki, recs, now_ns, mono, time_received, present, parts, rows, tab, held):
        """The merged flows through a LokiWriter; the filter's held flows (their stored Sampling does not fit the record) are taken out
        first and returned with their stored values."""
        n = len(recs)
        at = [j for j, _, _ in held]
        kept = np.delete(np.arange(n), at) if at else None
        take = (lambda a: a[kept] if a is not None else None) if at else (lambda a: a)
        sub_parts = {k: take(v) for k, v in parts.items()} if parts is not None else None
        bodies, late = loki.ExportEvicted(take(recs), now_ns, mono, time_received, present=take(present), parts=sub_parts, rows=take(rows), netev_table=tab)
        return bodies, [int(kept[i]) if at else i for i in late], held

    @staticmethod
    def _ipfix(ipfix, table, k8s, recs, now_ns, mono, present, parts, held):
        """The merged flows through a WriteIpfix; the filter's held flows are taken out first, as for Loki."""
        n = len(recs)
        at = [j for j, _, _ in held]
        kept = np.delete(np.arange(n), at) if at else None
        take = (lambda a: a[kept] if a is not None else None) if at else (lambda a: a)
        sub = take(recs)
        sub_parts = {k: take(v) for k, v in parts.items()} if parts is not None else None
        rows = table.k8s_resolve(k8s, sub) if k8s is not None and len(sub) else None
        sent = ipfix.Write(sub, now_ns, mono, present=take(present), parts=sub_parts, k8s_rows=rows)
        return sent, [(int(kept[i]) if at else i, st) for i, st in ipfix.failed], held

    def evictFlows(self, forwardFlows: "queue.Queue"):                  # :103-146
        monotonic_now, current = self.monoClock(), self.clock()
        flows = self.mapFetcher.LookupAndDeleteMap(self.metrics)
        udn_cache = dict(self.s.GetInterfaceUDNs()) if (self.s is not None and self.udnEnabled) else {}
        forwarding = [NewRecord(k, c.BpfFlowMetrics, current, monotonic_now, udn_cache,
                                dns_metrics=c.DNSMetrics, additional_metrics=c.AdditionalMetrics) for k, c in flows]
        self.mapFetcher.DeleteMapsStaleEntries(self.staleEntriesEvictTimeout)
        forwardFlows.put(forwarding)
        if self.metrics is not None:
            self.metrics.eviction("hashmap", "", len(forwarding))       # EvictionCounter / EvictedFlowsCounter WithSource("hashmap")
        return len(forwarding)


def NewMapTracer(fetcher, evictionTimeout, staleEntriesEvictTimeout, m=None, s=None, udnEnabled=False, **kw) -> MapTracer:
    return MapTracer(fetcher, evictionTimeout, staleEntriesEvictTimeout, m, s, udnEnabled, **kw)


def FlowsToPBMessages(buf, frame_offsets, max_len: int):
    """pbflow.FlowsToPB(records, maxLen) (pkg/pbflow/proto.go:18-36) over the output of nfagg_encode_pb: the serialized
    pbflow.Records messages GRPCProto.ExportFlows sends (pkg/exporter/grpc_proto.go:120), at most max_len entries each —
    byte ranges of `buf`, no copy of the frames' contents, no per-record allocation."""
    n = len(frame_offsets) - 1
    raw = memoryview(np.ascontiguousarray(buf))
    return [raw[int(frame_offsets[a]):int(frame_offsets[min(a + max_len, n)])] for a in range(0, n, max_len)]


class IPFIX:                                              # pkg/exporter/ipfix.go:33-42
    """The IPFIX exporter (EXPORT=ipfix+udp / ipfix+tcp) over the GPU encoder (FlowTable.encode_ipfix): evicted records go
    straight to IPFIX messages, no Record per flow. `send(message)` writes one message: one UDP datagram or one TCP write
    (the `send` of a socket the caller has connected; nothing here opens a socket). The state is go-ipfix's exporting
    process: seqNumber counts the data records sent (process.go:504-506), templates do not advance it.

    Differences from the reference, both by design: one Export Time per encode call (nfagg_encode_ipfix), and the UDP
    template refresh (every TempRefTimeout = 1 s, process.go:284-321) is sent in a fixed order, v4 then v6, before the
    first data message that finds 1 s or more passed since the last template send — the reference's ticker sends them in
    Go map order (random) from its own goroutine."""
    TEMPLATE_REFRESH_NS = 1_000_000_000

    def __init__(self, table, send: Callable, transport: str = "udp", names=None, unknown: bytes = b"unknown",
                 clock: Callable[[], int] = None, mono_clock: Callable[[], int] = None, obs_domain_id: int = 1, encode=None):
        if transport not in ("udp", "tcp"):
            raise ValueError("transport is 'udp' or 'tcp'")
        self.table, self.send, self.transport = table, send, transport
        self.names = names if names is not None else np.zeros(0, dtype=INTF_NAME)
        self.unknown, self.obsDomainID = unknown, obs_domain_id
        self.clock = clock or time.time_ns                # () -> unix ns (time.Now())
        self.monoClock = mono_clock or time.monotonic_ns  # () -> monotonic ns
        self.templateIDv4, self.templateIDv6 = IPFIX_TEMPLATE_ID_V4, IPFIX_TEMPLATE_ID_V6
        self.seqNumber = 0
        self.templatesSentAt = None
        # encode(raw, now_ns, mono_ns, names, export_time_s, seq0, unknown, obs_domain_id) -> (buf, msg_offsets)
        self._encode = encode or table.encode_ipfix

    def _export_time(self) -> int:                        # time.Now().Unix() as the message header's uint32
        return (self.clock() // 1_000_000_000) & 0xFFFFFFFF

    def sendTemplates(self):                              # SendTemplateRecordv4, SendTemplateRecordv6 (ipfix.go:240-251)
        self.templatesSentAt = self.clock()
        t = (self.templatesSentAt // 1_000_000_000) & 0xFFFFFFFF
        for v6 in (False, True):
            self.send(ipfix_template(v6, t, self.seqNumber, self.obsDomainID, (self.templateIDv4, self.templateIDv6)))

    def ExportEvicted(self, raw, now_ns: int, mono_ns: int) -> int:
        """sendDataRecord for every evicted record of one eviction (ipfix.go:364-383): encoded on the GPU, one message per flow.
        now_ns / mono_ns: the eviction's currentTime / monotonicCurrentTime (account.go:103-104). Returns the messages sent."""
        n = len(raw)
        if n == 0:
            return 0
        self._refresh()
        buf, off = self._encode(raw, now_ns, mono_ns & ((1 << 64) - 1), self.names, self._export_time(), self.seqNumber,
                                self.unknown, self.obsDomainID)
        raw_buf = memoryview(np.ascontiguousarray(buf))
        for i in range(n):
            if i:
                self._refresh()
            self.send(raw_buf[int(off[i]):int(off[i + 1])])
            self.seqNumber = (self.seqNumber + 1) & 0xFFFFFFFF
        return n

    def _refresh(self):
        if self.transport == "udp" and self.clock() - self.templatesSentAt >= self.TEMPLATE_REFRESH_NS:
            self.sendTemplates()

    def ExportFlows(self, inp: "queue.Queue"):            # ipfix.go:364-383: items (raw records, now_ns, mono_ns) until CLOSE
        while True:
            item = inp.get()
            if item is CLOSE:
                return
            raw, now_ns, mono_ns = item
            self.ExportEvicted(raw, now_ns, mono_ns)


def StartIPFIXExporter(table, send: Callable, transport: str = "udp", names=None, clock=None, mono_clock=None, **kw) -> IPFIX:
    """ipfix.go:220-262: the exporter, after it has sent the v4 template, then the v6 one."""
    ipf = IPFIX(table, send, transport, names=names, clock=clock, mono_clock=mono_clock, **kw)
    ipf.sendTemplates()
    return ipf


def _no_fallback(record, now_ns, mono_ns):
    raise NotImplementedError("TLS name tables (crypto/tls) stay with the Go decoder")


class DirectFLPJSON:                                      # pkg/exporter/direct_flp.go + write_stdout.go:37-51
    """The direct-FLP exporter in front of a lone `write: stdout, format: json` stage, over the GPU encoder
    (FlowTable.encode_flp_json): evicted records go straight to the JSON lines DirectFLPStdout prints, no Record and no dict
    per flow. Lines are written to `stream` (binary: anything with write(bytes)) in record order. A record the encoder
    defers (TLS version / cipher suite / key share set) is formatted by `fallback(record, now_ns, mono_ns) -> bytes`, the
    whole line with its newline, and written at its place; the default raises, as RecordToMap does for such a record.
    With `tls_names` (a TlsNames of `table`) the encoder writes those records' TLS keys itself (FlowTable.encode_flp_json_tls):
    nothing is deferred, `fallback` is never called and an eviction is one write. With `k8s` as well (a K8sTable of `table`; needs
    `tls_names`) the lines are those of the pipeline NetObserv ships, with the Kubernetes rules of its `transform network` stage in
    front of the writer (FlowTable.encode_flp_json_k8s). With `net` on top (a NetTable of `table`; needs `k8s`) the stage's
    reinterpret_direction, add_subnet_label and decode_tcp_flags rules are applied too (FlowTable.encode_flp_json_net), and no host pass
    over the lines is left. With `metrics` (a PromCounters or a PromMetrics; needs `k8s`) the `encode prom` metrics observe every
    eviction too (observe): the pipeline's other output, from the same records. Evicted records carry no feature parts, so a
    PromMetrics sees none here; MapTracer.evictFlowsJSON hands it those of its merged flows.

    One difference from the reference, by design: TimeReceived is read once per eviction, not once per flow."""

    def __init__(self, table, stream, names=None, agent_ip=None, unknown: bytes = b"unknown", time_received: Callable[[], int] = None,
                 fallback: Callable = None, encode=None, tls_names=None, k8s=None, net=None, metrics=None, filter=None, loki=None, ipfix=None):
        if loki is not None and net is None:
            raise ValueError("loki needs tls_names, k8s and net: the stage's labels are keys of the transform network stage")
        if k8s is not None and tls_names is None:
            raise ValueError("k8s needs tls_names: the enriched encoder defers nothing")
        if net is not None and k8s is None:
            raise ValueError("net needs k8s: reinterpret_direction reads the Kubernetes keys")
        if metrics is not None and k8s is None:
            raise ValueError("metrics needs k8s: the counters group by the Kubernetes keys")
        if filter is not None and tls_names is None:
            raise ValueError("filter needs tls_names: only a flow whose stored Sampling overflows is left to the fallback")
        # with a filter the fallback is called as fallback(record, now_ns, mono_ns, sampling=<the Sampling the reference stores>):
        # the record's 32 bits cannot carry it, so the record keeps its own and the line's value arrives beside it
        self.table, self.stream, self.metrics, self.filter = table, stream, metrics, filter
        self.names = names if names is not None else np.zeros(0, dtype=INTF_NAME)
        self.agent_ip, self.unknown = agent_ip, unknown
        self.time_received = time_received or (lambda: int(time.time()))   # time.Now().Unix()
        self.fallback = fallback or _no_fallback
        self.lines = self.deferred = 0
        # encode(raw, now_ns, mono_ns, names, agent_ip, time_received, unknown) -> (buf, line_offsets, deferred)
        self._encode = encode or table.encode_flp_json
        self.tls_names, self.k8s, self.net = tls_names, k8s, net
        # loki (a loki.LokiWriter over the same tables): the pipeline ends in `write loki` instead of `write stdout`. Nothing is
        # written to `stream`; the bodies go to the writer's send and stay in loki_bodies until the next eviction, loki_deferred
        # lists the flows of that eviction (positions among the kept) the caller formats itself, loki_held the filter's held flows
        # among them as (position, keep step, the Sampling the reference stores), what the stdout path hands its fallback.
        self.loki, self.loki_bodies, self.loki_deferred, self.loki_held = loki, [], [], []
        # ipfix (a flp_ipfix.WriteIpfix of `table`): the pipeline ends in `write ipfix`. Nothing is written to `stream`; the messages
        # go to the writer's send, ipfix_failed lists the flows of the last eviction that were not sent as (position, status),
        # ipfix_held the filter's held flows, which the writer does not see.
        self.ipfix, self.ipfix_failed, self.ipfix_held = ipfix, [], []

    def ExportEvicted(self, raw, now_ns: int, mono_ns: int) -> int:
        """One eviction's lines. now_ns / mono_ns: the eviction's currentTime / monotonicCurrentTime (account.go:103-104).
        Returns the lines written."""
        n = len(raw)
        if n == 0:
            return 0
        held = []
        if self.filter is not None:                       # `transform filter`: behind the resolves, in front of every encoder and fold
            raw, _, _, _, held = self.filter.apply(self.table, raw, self.k8s, self.net, self.agent_ip, now_ns, mono_ns)
            n = len(raw)
            if n == 0:
                return 0
        if self.metrics is not None:
            self.metrics.observe(self.table, raw, self.k8s, self.net, self.agent_ip)
        if self.loki is not None:                         # filter first, then conntrack's ids, then Loki (both inside the writer)
            held_at = [j for j, _, _ in held]
            kept = np.delete(np.arange(n), held_at) if held_at else np.arange(n)
            self.loki_bodies, late = self.loki.ExportEvicted(raw[kept] if held_at else raw, now_ns, mono_ns, self.time_received())
            self.loki_deferred, self.loki_held = sorted(held_at + [int(kept[i]) for i in late]), list(held)
            self.lines += n
            self.deferred += len(self.loki_deferred)
            return n
        if self.ipfix is not None:                        # filter first, then the Kubernetes rows, then the writer
            held_at = [j for j, _, _ in held]
            kept = np.delete(np.arange(n), held_at) if held_at else np.arange(n)
            sub = raw[kept] if held_at else raw
            rows = self.table.k8s_resolve(self.k8s, sub) if self.k8s is not None and len(sub) else None
            self.ipfix.Write(sub, now_ns, mono_ns, k8s_rows=rows)
            self.ipfix_failed, self.ipfix_held = [(int(kept[i]), st) for i, st in self.ipfix.failed], list(held)
            self.lines += n
            self.deferred += len(held)
            return n
        if self.tls_names is not None:
            if self.net is not None:
                buf, off = self.table.encode_flp_json_net(raw, self.tls_names, self.k8s, self.net, now_ns, mono_ns & ((1 << 64) - 1), self.names,
                                                          self.agent_ip, self.time_received(), self.unknown)
            elif self.k8s is not None:
                buf, off = self.table.encode_flp_json_k8s(raw, self.tls_names, self.k8s, now_ns, mono_ns & ((1 << 64) - 1), self.names,
                                                          self.agent_ip, self.time_received(), self.unknown)
            else:
                buf, off = self.table.encode_flp_json_tls(raw, self.tls_names, now_ns, mono_ns & ((1 << 64) - 1), self.names, self.agent_ip,
                                                          self.time_received(), self.unknown)
            raw_buf, start = memoryview(np.ascontiguousarray(buf)), 0
            for j, _, stored in held:                     # a kept flow whose stored Sampling needs more than 32 bits: the host's line
                self.stream.write(raw_buf[start:int(off[j])])
                self.stream.write(self.fallback(raw[j], now_ns, mono_ns, sampling=stored))
                start = int(off[j + 1])
            self.stream.write(raw_buf[start:int(off[n])])
            self.lines += n
            self.deferred += len(held)
            return n
        buf, off, deferred = self._encode(raw, now_ns, mono_ns & ((1 << 64) - 1), self.names, self.agent_ip, self.time_received(),
                                          self.unknown)
        raw_buf = memoryview(np.ascontiguousarray(buf))
        held = np.flatnonzero(deferred)
        start = 0
        for i in held:                                    # runs of encoded lines between deferred records: one write each
            i = int(i)
            if int(off[i]) > start:
                self.stream.write(raw_buf[start:int(off[i])])
            self.stream.write(self.fallback(raw[i], now_ns, mono_ns))
            start = int(off[i])
        if int(off[n]) > start:
            self.stream.write(raw_buf[start:int(off[n])])
        self.lines += n
        self.deferred += len(held)
        return n

    def ExportFlows(self, inp: "queue.Queue"):            # direct_flp.go ExportFlows: items (raw records, now_ns, mono_ns) until CLOSE
        while True:
            item = inp.get()
            if item is CLOSE:
                return
            raw, now_ns, mono_ns = item
            self.ExportEvicted(raw, now_ns, mono_ns)


def StartDirectFLPJSON(table, stream, names=None, agent_ip=None, **kw) -> DirectFLPJSON:
    """StartDirectFLP (direct_flp.go) with the `write: stdout, format: json` pipeline of direct_flp_test.go:17-33."""
    return DirectFLPJSON(table, stream, names=names, agent_ip=agent_ip, **kw)
