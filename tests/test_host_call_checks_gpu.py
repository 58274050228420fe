"""The first message of calls that break two or more rules at once, for the entry points that share the host-call vocabulary
(csrc/nfagg_api_call.h): write ipfix, write loki's plan and write, the transform filter and the gather, the conversation fold, the
Kubernetes and net resolves, the metrics folds and the conversation encoder. The entry points make their checks in different
orders on purpose and the first message is part of the C ABI; the texts here are literals of the source. No kernel runs in a
refused call. Also: what a host call answers for no records and for no room, and that write ipfix leaves no buffer behind."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

NOW, MONO = 1_700_000_000_123_456_789, 5_000_000_000
ENTRIES = [("10.0.0.1", dict(namespace="shop", name="cart-1", host_ip="192.168.0.1", host_name="node-a")),
           ("10.0.0.2", dict(namespace="bank", name="vault-2", host_ip="192.168.0.2", host_name="node-b"))]
V4MAP = bytes(10) + b"\xff\xff"
HANDLE = "was not created for this handle"


def flows(nf, n):
    """TCP flows 10.0.0.1 -> 10.0.0.2 with distinct ports."""
    r = np.zeros(n, dtype=nf.FLOW_RECORD)
    m, ids = r["metrics"], r["id"]
    m["eth_protocol"], ids["transport_protocol"] = 0x0800, 6
    for f, last in (("src_ip", 1), ("dst_ip", 2)):
        ids[f][:, :12] = np.frombuffer(V4MAP, dtype=np.uint8)
        ids[f][:, 12:] = (10, 0, 0, last)
    ids["src_port"], ids["dst_port"] = 1000 + np.arange(n), 443
    m["bytes"], m["packets"] = 100, 2
    m["start_mono_time_ts"], m["end_mono_time_ts"] = 1_000_000, 2_000_000
    m["if_index_first_seen"] = 2
    return r


class World:
    """One handle with a table of every kind, a second handle and host-only tables for the foreign ones, and device and host
    memory large enough for three records of anything, so that a call this file expects to be refused touches nothing it should
    not even if it were let through."""

    def __init__(self, nf):
        import torch
        self.nf, self.L = nf, nf._lib
        self.tab, self.other = nf.FlowTable(max_entries=64), nf.FlowTable(max_entries=64)
        t = self.tab
        self.tls, self.k8s, self.k8s2 = t.tls_names(), t.k8s_table(ENTRIES), t.k8s_table(ENTRIES)
        self.net, self.net_dir = t.net_table(), t.net_table(self.L.NET_REINTERPRET_DIRECTION)
        self.loki = t.loki_table(nf.WriteLoki(dict(timestampLabel="TimeFlowEndMs", timestampScale="1ms")), self.k8s, self.net)
        self.strings, self.writer = t.flp_ipfix_strings(ENTRIES), t.flp_ipfix_writer()
        self.flt = t.filter(nf.TransformFilter(None))
        rule = dict(type="keep_entry_query", keepEntryQuery='SrcK8S_Name = "cart-1"', keepEntrySampling=0)
        self.flt_k8s = t.filter(nf.TransformFilter(dict(rules=[rule]), k8s_entries=ENTRIES), self.k8s)
        self.met = t.metrics_table(self.k8s, [self.L.DIM_PROTO, self.L.DIM_SRC_SUBNET_LABEL])
        self.met_specs = t.metrics_table_specs(self.k8s, [dict(dims=self.L.DIM_PROTO)])
        self.layout = t.conn_layout([dict(name="Bytes", operation="sum", splitAB=True)])
        # foreign: built on the host only, or for the other handle
        self.f_k8s, self.f_net, self.f_tls = nf.K8sTable(ENTRIES), nf.NetTable(), nf.TlsNames()
        self.f_flt, self.f_layout = nf.Filter(nf.TransformFilter(None)), nf.ConnLayout([])
        self.f_met = nf.MetricsTable(self.f_k8s, [self.L.DIM_PROTO])
        self.f_strings, self.f_writer = nf.IpfixStrings(ENTRIES), self.other.flp_ipfix_writer()
        self.dev = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        self.d = self.dev.data_ptr()
        assert self.d % 256 == 0
        self.host = np.zeros(1 << 16, dtype=np.uint8)
        self.p = self.host.ctypes.data
        self.recs = flows(nf, 3)
        self.r = self.recs.ctypes.data
        self.dev[:3 * 144] = torch.from_numpy(self.recs.view(np.uint8).reshape(-1).copy())
        self.sz, self.sz2, self.u32a, self.u32b = C.c_size_t(7), C.c_size_t(7), C.c_uint32(7), C.c_uint32(7)
        self.closers = [self.f_writer, self.f_strings, self.f_met, self.f_layout, self.f_flt, self.f_tls, self.f_net, self.f_k8s, self.layout,
                        self.met_specs, self.met, self.flt_k8s, self.flt, self.writer, self.strings, self.loki, self.net_dir, self.net, self.k8s2,
                        self.k8s, self.tls, self.other, self.tab]

    def close(self):
        for c in self.closers:
            c.close()

    def refused(self, rc, code, text, h="tab"):
        handle = getattr(self, h)._h if h else None
        assert rc == code, (rc, self.L.lib.nfagg_last_error(handle))
        assert (self.L.lib.nfagg_last_error(handle) or b"").decode() == text

    def ipfix_opt(self, **kw):
        o, keep = self.nf.flp_ipfix_options(NOW, MONO, kw.pop("names", None), 1_700_000_123, 0, 2)
        for k, v in kw.items():
            setattr(o, k, v)
        return o, keep

    def flp_opt(self, **kw):
        o, keep = self.nf.flp_options(NOW, MONO, kw.pop("names", None), V4MAP + bytes([10, 0, 0, 9]))
        for k, v in kw.items():
            setattr(o, k, v)
        return o, keep

    def long_names(self, field):
        t = np.zeros(1, dtype=self.nf.INTF_NAME)
        t[field] = 17 if field == "name_len" else 64
        return t

    def bad_features(self):
        f = self.L.PbFeatures()
        f.struct_size = C.sizeof(self.L.PbFeatures) + 8
        return f


@pytest.fixture(scope="module")
def w(nf):
    world = World(nf)
    yield world
    world.close()


B = C.byref
EINVAL, ERANGE, OK, TRUNCATED = -1, -6, 0, 2


# ---- write ipfix
def test_flp_ipfix_write_device(w):
    f, h, d = w.L.lib.nfagg_flp_ipfix_write_device, w.tab._h, w.d
    o, _ = w.ipfix_opt(max_msg_size=70000)
    w.refused(f(h, w.writer._t, d, 1, None, None, None, B(o), d + 4096, 4096, d + 8192, d + 9000, B(w.sz), None), EINVAL, "max_msg_size 70000, more than 65535")
    o, keep = w.ipfix_opt(names=w.long_names("name_len"))
    w.refused(f(h, None, d, 1, None, None, None, B(o), d + 4096, 4096, d + 8192, d + 9000, B(w.sz), B(w.sz2)), EINVAL, "namer row 0: name too long")
    o, _ = w.ipfix_opt()
    w.refused(f(h, w.f_writer._t, d + 4, 1, None, None, None, B(o), d + 4096, 4096, d + 8192, d + 9000, B(w.sz), B(w.sz2)), EINVAL, "the writer " + HANDLE)
    w.refused(f(h, w.writer._t, d + 4, 2, None, d + 1024, None, B(o), d + 4096, 4096, d + 8192, d + 9000, B(w.sz), B(w.sz2)), EINVAL,
              "Kubernetes rows without the strings table they index")
    w.refused(f(h, w.writer._t, d, 2, None, d + 1024, w.f_strings._t, B(o), d + 4096, 4096, d + 8196, d + 9000, B(w.sz), B(w.sz2)), EINVAL,
              "the strings table " + HANDLE)
    bad = w.bad_features()
    w.refused(f(h, w.writer._t, d + 8, 3, B(bad), None, None, B(o), d + 4096, 4096, d + 8192, d + 9000, B(w.sz), B(w.sz2)), EINVAL,
              "device records and output must be 16-byte, rows and offsets 8-byte aligned")
    w.refused(f(h, w.writer._t, d, 3, B(bad), None, None, B(o), d + 4096, 4096, d + 8192, d + 9000, B(w.sz), B(w.sz2)), EINVAL,
              "nfagg_pb_features.struct_size mismatch")


def test_flp_ipfix_write_host(w):
    f, h, r, p = w.L.lib.nfagg_flp_ipfix_write, w.tab._h, w.r, w.p
    o, _ = w.ipfix_opt(struct_size=8)
    w.refused(f(h, w.writer._t, r, 1, None, None, None, B(o), p, 4096, None, p + 9000, B(w.sz), B(w.sz2)), EINVAL, "nfagg_flp_ipfix_options.struct_size mismatch")
    w.refused(f(h, w.writer._t, r, 1, None, None, None, None, p, 4096, None, p + 9000, B(w.sz), B(w.sz2)), EINVAL, "null options")
    o, _ = w.ipfix_opt()
    w.refused(f(h, w.f_writer._t, r, 1, None, None, None, B(o), p, 4096, p + 8192, None, B(w.sz), B(w.sz2)), EINVAL, "null argument")
    bad = w.bad_features()
    w.refused(f(h, w.f_writer._t, r, 1, B(bad), None, None, B(o), p, 4096, p + 8192, p + 9000, B(w.sz), B(w.sz2)), EINVAL, "the writer " + HANDLE)
    w.refused(f(h, w.writer._t, r, 2, B(bad), p + 1024, None, B(o), p, 4096, p + 8192, p + 9000, B(w.sz), B(w.sz2)), EINVAL, "nfagg_pb_features.struct_size mismatch")
    w.refused(f(h, w.writer._t, r, 2, None, p + 1024, None, B(o), p, 4096, p + 8192, p + 9000, B(w.sz), B(w.sz2)), EINVAL,
              "Kubernetes rows without the strings table they index")
    w.refused(f(h, w.writer._t, r, 2, None, p + 1024, w.f_strings._t, B(o), p, 4096, p + 8192, p + 9000, B(w.sz), B(w.sz2)), EINVAL, "the strings table " + HANDLE)


def test_flp_ipfix_write_no_records_no_room_and_no_buffer_left(nf, w):
    L = nf._lib
    start = nf.debug_live_buffers()
    tab = nf.FlowTable(max_entries=64)
    state, strings = tab.flp_ipfix_writer(), tab.flp_ipfix_strings(ENTRIES)
    try:
        o = nf.flp_ipfix_options(NOW, MONO, None, 1_700_000_123, 0, 2)
        rows = np.array([[0, 1]] * 3, dtype=np.uint32)
        rc, buf, off, status, sent = tab.flp_ipfix_write(state, w.recs[:0], o)
        assert (rc, len(buf), off.tolist(), len(status), sent) == (OK, 0, [0], 0, 0)
        before = [state.get(v6) for v6 in (False, True)]
        # no room: the host call's outputs stay as the caller left them, the sizes are answered, the state has not moved
        off, status, out = np.full(4, 77, dtype=np.uint64), np.full(3, 77, dtype=np.uint8), np.full(16, 77, dtype=np.uint8)
        need, n_sent = C.c_size_t(0), C.c_size_t(0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        args = (tab._h, state._t, ptr(w.recs), 3, None, ptr(rows), strings._t, B(o[0]))
        for out_p in (ptr(out), None):
            rc = L.lib.nfagg_flp_ipfix_write(*args, out_p, 0, ptr(off), ptr(status), B(n_sent), B(need))
            assert rc == TRUNCATED and n_sent.value == 3 and need.value > 3 * 20                # more than the headers alone
            assert off.tolist() == [77] * 4 and status.tolist() == [77] * 3 and out.tolist() == [77] * 16
        assert [state.get(v6) for v6 in (False, True)] == before
        rc, buf, off, status, sent = tab.flp_ipfix_write(state, w.recs, o, None, None, rows, strings)
        assert (rc, len(buf), int(off[3]), status.tolist(), sent) == (OK, need.value, need.value, [0, 0, 0], 3)
        assert nf.debug_live_buffers() > start
    finally:
        state.close()
        strings.close()
        tab.close()
    assert nf.debug_live_buffers() == start


# ---- write loki
def plan_args(w, **kw):
    """The arguments of nfagg_loki_plan_device behind the handle, valid for two records unless overridden."""
    a = dict(recs=w.d, n=2, feat=None, rows=None, netev=None, tls=w.tls._t, k8s=w.k8s._t, net=w.net._t, ids=None, opt=None, table=w.loki._t, now=NOW,
             streams=w.d + 8192, stream_cap=8, groups=w.d + 16384, group_cap=8, deferred=None, counts=None)
    a.update(kw)
    return tuple(a.values())


def test_loki_plan_device(w):
    f, h, d = w.L.lib.nfagg_loki_plan_device, w.tab._h, w.d
    counts = w.L.LokiCounts()
    o, _ = w.flp_opt()
    w.refused(f(h, *plan_args(w, opt=None, counts=None)), EINVAL, "null options")
    ou, keep = w.flp_opt(names=w.long_names("udn_len"))
    w.refused(f(h, *plan_args(w, opt=B(ou), tls=None, counts=B(counts))), EINVAL, "namer row 0: udn too long")
    w.refused(f(h, *plan_args(w, opt=B(o), table=None, rows=d + 1024, counts=B(counts))), EINVAL, "null argument")
    w.refused(f(h, *plan_args(w, opt=B(o), rows=d + 1024, k8s=w.f_k8s._t, counts=B(counts))), EINVAL, "network-events rows and table go together")
    w.refused(f(h, *plan_args(w, opt=B(o), k8s=w.f_k8s._t, recs=d + 4, counts=B(counts))), EINVAL, "the Kubernetes table " + HANDLE)
    w.refused(f(h, *plan_args(w, opt=B(o), k8s=w.k8s2._t, stream_cap=w.L.LOKI_MAX_STREAMS + 1, counts=B(counts))), EINVAL,
              "the Loki table was built over other tables than the call's")
    w.refused(f(h, *plan_args(w, opt=B(o), stream_cap=w.L.LOKI_MAX_STREAMS + 1, recs=d + 4, counts=B(counts))), ERANGE,
              "a cap of %u streams, more than %u" % (w.L.LOKI_MAX_STREAMS + 1, w.L.LOKI_MAX_STREAMS))
    w.refused(f(h, *plan_args(w, opt=B(o), recs=d + 4, ids=d + 1028, counts=B(counts))), EINVAL,
              "device records must be 16-byte, hash ids, streams and groups 8-byte aligned")


def host_plan_args(w, **kw):
    return plan_args(w, **dict(dict(recs=w.r, streams=w.p + 8192, groups=w.p + 16384), **kw))


def test_loki_plan_host(w):
    f, h = w.L.lib.nfagg_loki_plan, w.tab._h
    counts = w.L.LokiCounts()
    o, _ = w.flp_opt()
    big = w.L.LOKI_MAX_STREAMS + 1
    w.refused(f(h, *host_plan_args(w, opt=B(o), stream_cap=big, counts=None)), EINVAL, "null argument")
    bad = w.bad_features()
    w.refused(f(h, *host_plan_args(w, opt=B(o), stream_cap=big, feat=B(bad), counts=B(counts))), ERANGE, "a cap of %u streams, more than %u" % (big, big - 1))
    w.refused(f(h, *host_plan_args(w, opt=None, feat=B(bad), counts=B(counts))), EINVAL, "nfagg_pb_features.struct_size mismatch")
    w.refused(f(h, *host_plan_args(w, opt=None, tls=None, counts=B(counts))), EINVAL, "null options")
    w.refused(f(h, *host_plan_args(w, opt=B(o), tls=None, k8s=w.f_k8s._t, counts=B(counts))), EINVAL, "null argument")
    w.refused(f(h, *host_plan_args(w, opt=B(o), k8s=w.k8s2._t, net=w.f_net._t, counts=B(counts))), EINVAL, "the net table " + HANDLE)


def good_plan(w, n=2):
    counts = w.L.LokiCounts()
    o, _ = w.flp_opt()
    rc = w.L.lib.nfagg_loki_plan(w.tab._h, *host_plan_args(w, n=n, opt=B(o), counts=B(counts)))
    assert rc == OK, w.L.lib.nfagg_last_error(w.tab._h)
    return counts


NO_PLAN = "no plan: nfagg_loki_plan has not run on this handle, or its outputs were truncated"


def test_loki_write_device(w):
    f, d = w.L.lib.nfagg_loki_write_device, w.d
    w.refused(f(w.other._h, None, None, d + 4, 4096, d + 8192, d + 9000, None), EINVAL, "null argument", h="other")
    w.refused(f(w.other._h, None, None, d + 4, 4096, d + 8192, d + 9000, B(w.sz)), EINVAL, NO_PLAN, h="other")
    assert w.sz.value == 0
    h = w.tab._h
    counts = good_plan(w)
    assert counts.n_streams == 1 and counts.n_batches == 1
    off = np.array([0, 1], dtype=np.uint64)
    offp = off.ctypes.data
    w.refused(f(h, None, None, d + 4, 4096, d + 8192, d + 9000, B(w.sz)), EINVAL, "the output must be 16-byte, the batch offsets 8-byte aligned")
    w.refused(f(h, None, offp, d, 4096, d + 8192, None, B(w.sz)), EINVAL, "null label text")
    w.refused(f(h, b"{}", offp, d, 4096, d + 8192, None, B(w.sz)), EINVAL, "null argument")
    w.refused(f(h, b"{}", offp, None, 0, d + 8192, d + 9000, B(w.sz)), EINVAL, "stream 0: a label text of 1 bytes, not 2 .. %u" % w.L.LOKI_LABELS_MAX)


def test_loki_write_host_no_records_and_no_room(w):
    f, p = w.L.lib.nfagg_loki_write, w.p
    w.refused(f(w.other._h, None, None, p, 4096, None, p + 9000, B(w.sz)), EINVAL, "null argument", h="other")
    w.refused(f(w.other._h, None, None, p, 4096, p + 8192, None, B(w.sz)), EINVAL, NO_PLAN, h="other")
    h = w.tab._h
    good_plan(w)
    off = np.array([0, 2], dtype=np.uint64)
    offp = off.ctypes.data
    w.refused(f(h, None, None, p, 4096, p + 8192, None, B(w.sz)), EINVAL, "null argument")
    w.refused(f(h, None, offp, p, 4096, p + 8192, p + 9000, B(w.sz)), EINVAL, "null label text")
    # no room: the batch offsets and entries are answered with the size
    boff, bent = np.full(2, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint32)
    rc = f(h, b"{}", offp, None, 0, boff.ctypes.data, bent.ctypes.data, B(w.sz))
    assert rc == TRUNCATED and w.sz.value > 4 and boff.tolist() == [0, w.sz.value] and bent.tolist() == [2]
    out = np.zeros(w.sz.value, dtype=np.uint8)
    assert f(h, b"{}", offp, out.ctypes.data, out.size, boff.ctypes.data, bent.ctypes.data, B(w.sz2)) == OK and w.sz2.value == out.size
    # no records: a plan of nothing, and a write of nothing
    counts = good_plan(w, n=0)
    assert (counts.n_streams, counts.n_groups, counts.n_batches, counts.n_deferred) == (0, 0, 0, 0)
    boff[:] = 77
    assert f(h, None, None, None, 0, boff.ctypes.data, None, B(w.sz)) == OK and w.sz.value == 0 and boff.tolist() == [0, 77]


# ---- transform filter, gather
def test_filter_apply_device(w):
    f, h, d = w.L.lib.nfagg_filter_apply_device, w.tab._h, w.d
    tail = (0, 0, d + 4096, d + 4200, d + 4400, d + 8192, 3)
    w.refused(f(h, w.f_flt._t, d, 3, None, None, None, None, *tail, None, None), EINVAL, "null argument")
    w.refused(f(h, w.f_flt._t, d + 4, 3, None, None, None, None, *tail, B(w.sz), None), EINVAL, "the filter " + HANDLE)
    assert w.sz.value == 0
    w.refused(f(h, w.flt_k8s._t, d + 4, 3, None, None, None, None, *tail, B(w.sz), None), EINVAL, "the filter reads the flows' Kubernetes rows")
    bad = w.bad_features()
    w.refused(f(h, w.flt._t, d + 4, 3, B(bad), None, None, None, *tail, B(w.sz), None), EINVAL, "nfagg_pb_features.struct_size mismatch")
    w.refused(f(h, w.flt._t, d, 3, None, None, None, None, 0, 0, d + 4096, d + 4200, d + 4402, d + 8192, 3, B(w.sz), None), EINVAL,
              "device records must be 16-byte, rows 8-byte, kept_idx 4-byte aligned")


def test_filter_apply_host_no_records_and_no_room(nf, w):
    f, h, r, p = w.L.lib.nfagg_filter_apply, w.tab._h, w.r, w.p
    tail = (0, 0, p + 4096, p + 4200, p + 4400, p + 8192, 3)
    w.refused(f(h, None, r, 3, B(w.bad_features()), None, None, None, *tail, B(w.sz), None), EINVAL, "null argument")
    w.refused(f(h, w.f_flt._t, r, 3, B(w.bad_features()), None, None, None, *tail, B(w.sz), None), EINVAL, "nfagg_pb_features.struct_size mismatch")
    w.refused(f(h, w.f_flt._t, r, 3, None, None, None, None, *tail, B(w.sz), None), EINVAL, "the filter " + HANDLE)
    w.refused(f(h, w.flt_k8s._t, r, 3, None, None, p + 1024, None, *tail, B(w.sz), None), EINVAL, "the filter reads the flows' Kubernetes rows")
    rc, keep, rule, idx, out, n_kept, n_def = w.tab.filter_apply(w.flt, w.recs[:0])
    assert (rc, len(keep), len(idx), n_kept, n_def) == (OK, 0, 0, 0, 0)
    keep = np.zeros(3, dtype=np.uint8)                                                              # no rule: every flow is kept, and there is room for none
    assert f(h, w.flt._t, r, 3, None, None, None, None, 0, 0, keep.ctypes.data, p + 4200, p + 4400, p + 8192, 0, B(w.sz), B(w.sz2)) == TRUNCATED
    assert (w.sz.value, w.sz2.value) == (3, 0) and keep.all()
    rc, keep, rule, idx, out, n_kept, n_def = w.tab.filter_apply(w.flt, w.recs)
    assert (rc, idx.tolist(), n_kept) == (OK, [0, 1, 2], 3) and out.tobytes() == w.recs.tobytes()


def test_gather_host(w):
    f, h, p = w.L.lib.nfagg_gather, w.tab._h, w.p
    w.refused(f(h, p, 4, 3, None, 2, None), EINVAL, "gather of 3-byte elements: not 1, 2, 4, 8 or a multiple of 8 up to 64")
    w.refused(f(None, p, 4, 3, None, 2, None), EINVAL, "null argument", h=None)
    w.refused(f(h, None, 4, 8, p + 1024, 2, None), EINVAL, "null argument")
    assert f(h, p, 4, 8, None, 0, None) == OK                     # nothing kept: nothing is staged
    src = np.arange(5, dtype=np.uint64)
    assert w.tab.gather(src, np.array([4, 0, 9], dtype=np.uint32)).tolist() == [4, 0, 0]


# ---- conversation fold
def conn_opt(w, struct_size=None):
    o = w.L.ConnOptions(struct_size=C.sizeof(w.L.ConnOptions), now_unix_ns=NOW, mono_now_ns=MONO)
    if struct_size is not None:
        o.struct_size = struct_size
    return o


def test_conn_fold_device(w):
    f, h, d = w.L.lib.nfagg_conn_fold_device, w.tab._h, w.d
    big = w.L.CONN_MAX_CONNS + 1
    o, bad = conn_opt(w), conn_opt(w, 8)
    w.refused(f(h, d, 3, None, d + 1024, big, d + 4096, B(w.u32a), B(w.u32b)), EINVAL, "null argument")
    w.refused(f(h, d, 3, B(bad), d + 1024, big, d + 4096, B(w.u32a), B(w.u32b)), EINVAL, "nfagg_conn_options.struct_size mismatch")
    w.refused(f(h, d, 3, B(o), d + 1024, big, None, B(w.u32a), B(w.u32b)), ERANGE, "a cap of %u connections, more than %u" % (big, big - 1))
    w.refused(f(h, d + 4, 3, B(o), d + 1024, 8, None, B(w.u32a), B(w.u32b)), EINVAL, "a cap without an output array")
    w.refused(f(h, d, 3, B(o), d + 1028, 8, d + 4096, B(w.u32a), B(w.u32b)), EINVAL, "device records and partials must be 16-byte, hash ids 8-byte aligned")


def test_conn_fold_host_no_records_and_no_room(w):
    f, h, r, p = w.L.lib.nfagg_conn_fold, w.tab._h, w.r, w.p
    big = w.L.CONN_MAX_CONNS + 1
    o, bad = conn_opt(w), conn_opt(w, 8)
    w.refused(f(h, r, 3, B(bad), p + 1024, big, p + 4096, None, B(w.u32b)), EINVAL, "null argument")
    w.refused(f(h, r, 3, B(bad), p + 1024, big, None, B(w.u32a), B(w.u32b)), ERANGE, "a cap of %u connections, more than %u" % (big, big - 1))
    w.refused(f(h, r, 3, B(bad), p + 1024, 8, None, B(w.u32a), B(w.u32b)), EINVAL, "a cap without an output array")
    w.refused(f(h, r, 3, B(bad), p + 1024, 8, p + 4096, B(w.u32a), B(w.u32b)), EINVAL, "nfagg_conn_options.struct_size mismatch")
    rc, out, n_conns, ids, n_disc = w.tab.conn_fold(w.recs[:0], NOW, MONO)
    assert (rc, len(out), n_conns, len(ids), n_disc) == (OK, 0, 0, 0, 0)
    rc, out, n_conns, ids, n_disc = w.tab.conn_fold(w.recs, NOW, MONO, cap=0)                       # three connections, room for none
    assert (rc, len(out)) == (TRUNCATED, 0) and n_conns >= 1
    rc, out, n_conns, ids, n_disc = w.tab.conn_fold(w.recs, NOW, MONO)
    assert (rc, len(out), n_conns, n_disc) == (OK, 3, 3, 0) and ids.all()


# ---- the resolves
def test_k8s_resolve_host(w):
    f, h, r, p = w.L.lib.nfagg_k8s_resolve, w.tab._h, w.r, w.p
    w.refused(f(h, None, r, 1, None), EINVAL, "null argument")
    w.refused(f(h, w.f_k8s._t, r, 1, None), EINVAL, "null argument")
    w.refused(f(h, w.f_k8s._t, r, 1, p), EINVAL, "the Kubernetes table " + HANDLE)
    w.refused(f(h, w.f_k8s._t, None, 0, None), EINVAL, "the Kubernetes table " + HANDLE)
    assert f(h, w.k8s._t, None, 0, None) == OK
    assert np.asarray(w.tab.k8s_resolve(w.k8s, w.recs)).reshape(-1, 2).tolist() == [[0, 1]] * 3


def test_net_resolve_host(w):
    f, h, r, p = w.L.lib.nfagg_net_resolve, w.tab._h, w.r, w.p
    need = "reinterpret_direction needs the Kubernetes table, the flows' rows and the options"
    o, bad = w.flp_opt()[0], w.flp_opt(struct_size=8)[0]
    w.refused(f(h, None, w.f_k8s._t, r, 1, None, None, p), EINVAL, "null argument")
    w.refused(f(h, w.net_dir._t, None, r, 1, None, None, None), EINVAL, "null argument")
    w.refused(f(h, w.net_dir._t, None, r, 1, None, B(bad), p), EINVAL, need)
    w.refused(f(h, w.f_net._t, None, r, 1, p + 1024, None, p), EINVAL, "the net table " + HANDLE)
    w.refused(f(h, w.net_dir._t, None, r, 1, p + 1024, B(bad), p), EINVAL, need)
    w.refused(f(h, w.net_dir._t, w.f_k8s._t, r, 1, p + 1024, B(bad), p), EINVAL, "nfagg_flp_options.struct_size mismatch")
    w.refused(f(h, w.net_dir._t, w.f_k8s._t, r, 1, p + 1024, B(o), p), EINVAL, "the Kubernetes table " + HANDLE)
    w.refused(f(h, w.net_dir._t, None, None, 0, None, None, None), EINVAL, need)                    # no records: the tables are still checked
    assert f(h, w.net._t, None, None, 0, None, None, None) == OK


# ---- metrics
def fold_args(w, caps, outs):
    G = len(caps)
    return (C.c_uint32 * G)(*caps), (C.c_void_p * G)(*outs), (C.c_uint32 * G)(*([7] * G))


def test_metrics_fold_host_and_content(w):
    L, h, r, p = w.L, w.tab._h, w.r, w.p
    f, fc = L.lib.nfagg_metrics_fold, L.lib.nfagg_metrics_fold_content
    big = L.MET_MAX_GROUPS + 1
    cap, out, n = fold_args(w, [big, 8], [None, None])
    w.refused(f(h, w.met._t, r, 3, p + 1024, None, cap, out, None), EINVAL, "null argument")
    w.refused(f(h, w.f_met._t, r, 3, p + 1024, None, cap, out, n), ERANGE, "grouping 0: a cap of %u groups, more than %u" % (big, big - 1))
    cap, out, n = fold_args(w, [8, 8], [p + 4096, None])
    w.refused(f(h, w.met._t, r, 3, p + 1024, None, cap, out, n), EINVAL, "grouping 1: a cap without an output array")
    cap, out, n = fold_args(w, [8], [p + 4096])
    w.refused(f(h, w.f_met._t, r, 3, p + 1024, None, cap, out, n), EINVAL, "the metrics table " + HANDLE)
    w.refused(f(h, w.met_specs._t, r, 3, p + 1024, None, cap, out, n), EINVAL, "the metrics table was created from specs: use nfagg_metrics_fold_content")
    cap, out, n = fold_args(w, [8, 8], [p + 4096, p + 8192])
    w.refused(f(h, w.met._t, r, 3, p + 1024, None, cap, out, n), EINVAL, "grouping 1 selects a label or the direction: it needs the flows' net rows")
    bad = w.bad_features()
    cap, out, n = fold_args(w, [big], [p + 4096])
    w.refused(fc(h, w.met_specs._t, r, 3, B(bad), p + 1024, None, cap, out, None), EINVAL, "null argument")
    w.refused(fc(h, w.met_specs._t, r, 3, B(bad), p + 1024, None, cap, out, n), EINVAL, "nfagg_pb_features.struct_size mismatch")
    w.refused(fc(h, w.met_specs._t, r, 3, None, p + 1024, None, cap, out, n), ERANGE, "grouping 0: a cap of %u groups, more than %u" % (big, big - 1))
    # no records: zero groups in every grouping; no room: the counts, above the cap where the grouping overflowed
    rows = np.array([[0, 1]] * 3, dtype=np.uint32)
    rc, groups, counts = w.tab.metrics_fold_content(w.met_specs, w.recs[:0], rows[:0])
    assert (rc, counts, [len(g) for g in groups]) == (OK, [0], [0])
    rc, groups, counts = w.tab.metrics_fold_content(w.met_specs, w.recs, rows, caps=0)
    assert (rc, counts, [len(g) for g in groups]) == (TRUNCATED, [1], [0])
    rc, groups, counts = w.tab.metrics_fold_content(w.met_specs, w.recs, rows)
    assert (rc, counts, [len(g) for g in groups]) == (OK, [1], [1])


# ---- conversation records
def test_encode_conn_json_host_no_records_and_no_room(nf, w):
    f, h, r, p = w.L.lib.nfagg_encode_conn_json, w.tab._h, w.r, w.p
    tail = (p + 4096, 4096, p + 8192, None, None, B(w.sz))
    w.refused(f(h, r, p + 1024, 2, None, w.f_k8s._t, w.net._t, *tail), EINVAL, "null argument")
    w.refused(f(h, r, None, 2, w.f_layout._t, w.f_k8s._t, w.net._t, *tail), EINVAL, "null argument")
    w.refused(f(h, r, p + 1024, 2, w.f_layout._t, w.f_k8s._t, w.net._t, *tail), EINVAL, "the layout " + HANDLE)
    w.refused(f(h, r, p + 1024, 2, w.layout._t, w.f_k8s._t, w.f_net._t, *tail), EINVAL, "the Kubernetes table " + HANDLE)
    w.refused(f(h, r, p + 1024, 2, w.layout._t, w.k8s._t, w.f_net._t, *tail), EINVAL, "the net table " + HANDLE)
    w.refused(f(h, None, None, 0, w.layout._t, w.k8s._t, w.f_net._t, *tail), EINVAL, "the net table " + HANDLE)
    values = np.zeros(2, dtype=nf.CONN_VALUES)
    off, need, n_def = np.full(3, 77, dtype=np.uint64), C.c_size_t(7), C.c_size_t(7)
    assert f(h, None, None, 0, w.layout._t, w.k8s._t, w.net._t, p + 4096, 4096, off.ctypes.data, None, B(n_def), B(need)) == OK
    assert (need.value, n_def.value, off.tolist()) == (0, 0, [0, 77, 77])
    args = (h, r, values.ctypes.data, 2, w.layout._t, w.k8s._t, w.net._t)
    assert f(*args, p + 4096, 0, off.ctypes.data, None, B(n_def), B(need)) == TRUNCATED and need.value > 2 * 2 and n_def.value == 0
    total = need.value
    assert f(*args, p + 4096, total, off.ctypes.data, None, B(n_def), B(need)) == OK and need.value == total and int(off[2]) == total and int(off[0]) == 0
    assert w.host[4096:4097].tobytes() == b"{" and w.host[4096 + total - 1:4096 + total].tobytes() == b"\n"
