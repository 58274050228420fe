"""flowlogs-pipeline's `write ipfix` stage over the device path (include/nfagg.h, "write ipfix on the device").

WriteIpfix mirrors NewWriteIpfix (pkg/pipeline/write/write_ipfix.go:582-648): the parameters of api.WriteIpfix with their
defaults and checks, the two template messages sent at start, the exporter's sequence number, the element state of both
families (on the device, in an IpfixWriterState). It works over the caller's send(message) and opens no socket, as pipeline.IPFIX
does. IpfixStrings is the three strings the stage reads of every Kubernetes row (nfagg_flp_ipfix_strings_create);
flp_ipfix_write is the one call."""
import ctypes as C

import numpy as np

from . import _lib as L
from .loki import parse_duration
from .records import INTF_NAME
from .table import (IPFIX_TEMPLATE_ID_V4, IPFIX_TEMPLATE_ID_V6, NfaggError, _CallerTable, _encode_options, _k8s_entry)

STATUS_NAMES = {L.FLP_IPFIX_SENT: "sent", L.FLP_IPFIX_FAIL_FAMILY: "address family", L.FLP_IPFIX_FAIL_SIZE: "message size"}
STRING_NAMES = ("interfaceName", "sourcePodNamespace", "sourcePodName", "destinationPodNamespace", "destinationPodName", "sourceNodeName",
                "destinationNodeName", "interfaces", "directions")
MAX_MSG_UDP, MAX_MSG_TCP = 512, 65535           # exporter/process.go:121-158 without a PMTU or a requested size


def flp_ipfix_options(now_unix_ns=0, mono_now_ns=0, names=None, export_time_s=0, seq0=0, enterprise_id=0, max_msg_size=MAX_MSG_TCP,
                      flags_decoded=False, unknown=b"unknown", obs_domain_id=1, template_ids=(IPFIX_TEMPLATE_ID_V4, IPFIX_TEMPLATE_ID_V6)):
    """nfagg_flp_ipfix_options; returns (options, the names array the options point into: keep it alive for the call)."""
    o, names = _encode_options(L.FlpIpfixOptions, now_unix_ns, mono_now_ns, names, unknown)
    o.export_time_s, o.seq0, o.obs_domain_id = export_time_s & 0xFFFFFFFF, seq0 & 0xFFFFFFFF, obs_domain_id
    o.template_id_v4, o.template_id_v6 = template_ids
    o.enterprise_id, o.max_msg_size, o.flags_decoded = enterprise_id, max_msg_size, 1 if flags_decoded else 0
    return o, names


def flp_ipfix_template(v6: bool, export_time_s: int = 0, seq: int = 0, enterprise_id: int = 0, obs_domain_id: int = 1,
                       template_ids=(IPFIX_TEMPLATE_ID_V4, IPFIX_TEMPLATE_ID_V6)) -> bytes:
    """nfagg_flp_ipfix_template: the template message of a family. Host only."""
    o, _ = flp_ipfix_options(export_time_s=export_time_s, seq0=seq, enterprise_id=enterprise_id, obs_domain_id=obs_domain_id,
                             template_ids=template_ids)
    buf = (C.c_uint8 * 256)()
    n = C.c_size_t(0)
    rc = L.lib.nfagg_flp_ipfix_template(C.byref(o), 1 if v6 else 0, buf, len(buf), C.byref(n))
    if rc != L.OK:
        raise NfaggError(rc, (L.lib.nfagg_last_error(None) or b"").decode())
    return bytes(buf[: n.value])


class IpfixStrings(_CallerTable):
    """nfagg_flp_ipfix_strings_create: entries as K8sTable takes them (row r is entries[r], so k8s_resolve's rows index it). With
    a FlowTable the table lives on its device and serves flp_ipfix_write; with table=None it is built and checked on the host."""

    def __init__(self, entries, table=None):
        entries = list(entries)
        made = [_k8s_entry(ip, info) for ip, info in entries]
        arr = (L.K8sEntry * max(len(made), 1))(*[e for e, _ in made])
        self._create(table, L.lib.nfagg_flp_ipfix_strings_destroy, lambda h, out: L.lib.nfagg_flp_ipfix_strings_create(h, arr, len(made), out))
        self.n, self.entries = len(made), entries

    def __len__(self):
        return self.n


class IpfixWriterState(_CallerTable):
    """nfagg_flp_ipfix_writer_create: the element state of both families on a FlowTable's device."""

    def __init__(self, table):
        self._create(table, L.lib.nfagg_flp_ipfix_writer_destroy, lambda h, out: L.lib.nfagg_flp_ipfix_writer_create(h, out))

    def get(self, v6: bool) -> dict:
        """The family's element values: numbers, addresses and MACs as bytes (None while still nil), strings by element name."""
        e = L.FlpIpfixElements()
        self._owner._check(L.lib.nfagg_flp_ipfix_writer_get(self._t, 1 if v6 else 0, C.byref(e)))
        out = {k: getattr(e, k) for k in ("proto", "icmp_type", "icmp_code", "flow_direction", "etype", "src_port", "dst_port", "flags",
                                          "xlat_src_port", "xlat_dst_port", "selector_algorithm", "bytes", "packets", "start_ms", "end_ms",
                                          "rtt_ns", "sampling_probability")}
        out["src_addr"], out["dst_addr"] = (bytes(e.src_addr), bytes(e.dst_addr)) if e.addr_set else (None, None)
        out["xlat_src_addr"], out["xlat_dst_addr"] = (bytes(e.xlat_src_addr), bytes(e.xlat_dst_addr)) if e.xlat_set else (None, None)
        out["src_mac"], out["dst_mac"] = (bytes(e.src_mac), bytes(e.dst_mac)) if e.mac_set else (None, None)
        for k, name in enumerate(STRING_NAMES):
            out[name] = bytes(e.str[k][: e.str_len[k]])
        return out

    def reset(self):
        self._owner._check(L.lib.nfagg_flp_ipfix_writer_reset(self._t))


def flp_ipfix_write(table, state: IpfixWriterState, records, options, present=None, parts=None, k8s_rows=None, strings: IpfixStrings = None,
                    out_cap: int = None):
    """nfagg_flp_ipfix_write. options: flp_ipfix_options(...). present / parts: the feature parts of full flow contents (None:
    records that carry only BpfFlowMetrics); k8s_rows: 2 x n rows as k8s_resolve returns them, indexing `strings`. Returns
    (rc, buf, msg_offsets, status, n_sent); the buffer grows until the messages fit unless out_cap is given (then rc may be
    L.TRUNCATED: buf holds nothing, msg_offsets[-1] what is needed, and the state has not moved)."""
    r = np.ascontiguousarray(records)
    n = r.nbytes // 144
    o, keep = options
    feat = keep_f = None
    if present is not None:
        feat, keep_f = table._pb_features(n, present, table._content_parts(parts))
    rw = np.ascontiguousarray(k8s_rows, dtype=np.uint32).reshape(n, 2) if k8s_rows is not None else None
    off, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8)
    need, sent = C.c_size_t(0), C.c_size_t(0)
    cap = int(out_cap) if out_cap is not None else 0
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None  # noqa: E731
    while True:
        buf = np.zeros(max(cap, 16), dtype=np.uint8)
        rc = L.lib.nfagg_flp_ipfix_write(table._h, state._t, ptr(r), n, C.byref(feat) if feat is not None else None, ptr(rw),
                                         strings._t if strings is not None else None, C.byref(o), ptr(buf), cap, ptr(off),
                                         ptr(status), C.byref(sent), C.byref(need))
        table._check(rc, ok=(L.OK, L.TRUNCATED))
        if rc == L.OK or out_cap is not None:
            break
        cap = need.value
    if rc != L.OK:
        off[-1] = need.value
    return rc, buf[: need.value if rc == L.OK else 0], off, status[:n], sent.value


class WriteIpfix:
    """The stage. config: the api.WriteIpfix keys as the YAML has them (targetHost, targetPort, transport, enterpriseId,
    tplSendInterval). send(message) takes every message in order: the two templates at start (sendTemplates), then one per sent
    flow. The caller owns the clock: Write(..., now_s) stamps the call's messages and, over UDP, sends the templates again first
    once tplSendInterval has passed since they were last sent (go-ipfix refreshes templates for UDP collectors only). failed:
    the (flow index, status) of the last Write's flows that were not sent."""

    def __init__(self, table, config: dict, send, strings: IpfixStrings = None, names=None, unknown: bytes = b"unknown",
                 flags_decoded: bool = False, now_s: int = 0, max_msg_size: int = None):
        c = dict(config or {})
        self.target_host, self.target_port = c.get("targetHost", ""), int(c.get("targetPort") or 0)
        self.transport = c.get("transport") or "tcp"                                 # SetDefaults
        interval = c.get("tplSendInterval") or "1m"
        self.tpl_send_interval_s = parse_duration(interval) // 10 ** 9 if isinstance(interval, str) else int(interval)
        self.enterprise_id = int(c.get("enterpriseId") or 0)
        if not self.target_host:                                                     # Validate
            raise ValueError("targetHost can't be empty")
        if not self.target_port:
            raise ValueError("targetPort can't be empty")
        if self.transport not in ("tcp", "udp"):
            raise ValueError("transport should be tcp/udp")
        self.max_msg_size = int(max_msg_size) if max_msg_size else (MAX_MSG_TCP if self.transport == "tcp" else MAX_MSG_UDP)
        self.table, self.send, self.strings = table, send, strings
        self.names = names if names is not None else np.zeros(0, dtype=INTF_NAME)
        self.unknown, self.flags_decoded = unknown, flags_decoded
        self.template_ids = (IPFIX_TEMPLATE_ID_V4, IPFIX_TEMPLATE_ID_V6)              # NewTemplateID twice, from 255
        self.state = IpfixWriterState(table)
        self.seqNumber = 0
        self.failed = []
        self.sendTemplates(now_s)

    def sendTemplates(self, now_s: int):
        for v6 in (False, True):
            self.send(flp_ipfix_template(v6, now_s, self.seqNumber, self.enterprise_id, 1, self.template_ids))
        self._templates_at = now_s

    def Write(self, raw, now_ns: int, mono_ns: int, now_s: int = None, present=None, parts=None, k8s_rows=None, strings: IpfixStrings = None):
        """One eviction's flows through the stage. Returns the number of flows sent."""
        now_s = int(now_ns // 10 ** 9) if now_s is None else int(now_s)
        if self.transport == "udp" and now_s - self._templates_at >= max(self.tpl_send_interval_s, 1):
            self.sendTemplates(now_s)
        n = len(raw)
        self.failed = []
        if n == 0:
            return 0
        o = flp_ipfix_options(now_ns, mono_ns & ((1 << 64) - 1), self.names, now_s, self.seqNumber, self.enterprise_id, self.max_msg_size,
                              self.flags_decoded, self.unknown, 1, self.template_ids)
        rc, buf, off, status, sent = flp_ipfix_write(self.table, self.state, raw, o, present, parts, k8s_rows,
                                                     strings if strings is not None else self.strings)
        view = memoryview(np.ascontiguousarray(buf))
        for i in range(n):
            if status[i] == L.FLP_IPFIX_SENT:
                self.send(bytes(view[int(off[i]):int(off[i + 1])]))
            else:
                self.failed.append((i, int(status[i])))
        self.seqNumber = (self.seqNumber + sent) & 0xFFFFFFFF
        return sent

    def close(self):
        self.state.close()
