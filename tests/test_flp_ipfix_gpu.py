"""write ipfix on the device (nfagg_flp_ipfix_write; csrc/nfagg_flp_ipfix.hip) through the C ABI, host and device entry points.
Bytes, offsets, status, n_sent and the read-back element state are compared with the restatement of tests/flp_ipfix_ref.py over
the maps of tests/flp_json_content_ref.py and flp_json_k8s_ref.py; every sent message is also decoded by the template the product
wrote. The bytes are pinned to that restatement and go-ipfix's source, not to a Go run. Shapes are the smallest at which a path
can go wrong: a wave is 64 flows, a block 1024, the scan over blocks gives a thread more than one block from 2^16 flows on."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_ipfix_ref as R  # noqa: E402
import flp_json_k8s_ref as K  # noqa: E402
import test_flp_json_content_gpu as CG  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
import test_flp_json_k8s_gpu as KG  # noqa: E402
import test_netev_gpu as E  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, NOW, MONO = G.NAMES, G.NOW, G.MONO
EXPORT = 1_700_000_123
V4MAP = bytes(10) + b"\xff\xff"
# element name -> key of IpfixWriterState.get(); the address and ICMP elements by family
STATE_KEYS = {"ethernetType": "etype", "flowDirection": "flow_direction", "sourceMacAddress": "src_mac", "destinationMacAddress": "dst_mac",
              "protocolIdentifier": "proto", "sourceTransportPort": "src_port", "destinationTransportPort": "dst_port", "octetDeltaCount": "bytes",
              "flowStartMilliseconds": "start_ms", "flowEndMilliseconds": "end_ms", "packetDeltaCount": "packets", "tcpControlBits": "flags",
              "postNAPTSourceTransportPort": "xlat_src_port", "postNAPTDestinationTransportPort": "xlat_dst_port",
              "selectorAlgorithm": "selector_algorithm", "samplingProbability": "sampling_probability", "timeFlowRttNs": "rtt_ns",
              "nextHeaderIPv6": "proto"}
for _v in ("4", "6"):
    STATE_KEYS.update({"sourceIPv%sAddress" % _v: "src_addr", "destinationIPv%sAddress" % _v: "dst_addr", "icmpTypeIPv" + _v: "icmp_type",
                       "icmpCodeIPv" + _v: "icmp_code", "postNATSourceIPv%sAddress" % _v: "xlat_src_addr",
                       "postNATDestinationIPv%sAddress" % _v: "xlat_dst_addr"})


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


class Pair:
    """The product's writer state and the restatement's writer, fed the same calls."""

    def __init__(self, nf, tab, enterprise=2, max_msg=65535, flags_decoded=False):
        self.nf, self.tab, self.enterprise, self.max_msg, self.flags_decoded = nf, tab, enterprise, max_msg, flags_decoded
        self.state = tab.flp_ipfix_writer()
        self.ref = R.WriteIpfix(lambda m: None, enterprise, max_msg)
        self.templates = dict(R.parse_template(nf.flp_ipfix_template(v6, EXPORT, 0, enterprise)) for v6 in (False, True))
        self.seq = 0
        self.sent = []                                            # every message the product wrote, in order

    def close(self):
        self.state.close()

    def options(self):
        return self.nf.flp_ipfix_options(NOW, MONO, G.table(self.nf, NAMES), EXPORT, self.seq, self.enterprise, self.max_msg, self.flags_decoded)

    def check_state(self):
        for v6 in (False, True):
            got, want = self.state.get(v6), self.ref.elements(v6)
            for name, value in want.items():
                g = got[STATE_KEYS[name]] if name in STATE_KEYS else got[name]
                if name.endswith("Address") and "Mac" not in name:
                    value = R.to16(value)
                assert g == value, (v6, name, g, value)

    def call(self, recs, present=None, parts=None, entries=None, strings=None, device=False, only=None):
        """One call through the host entry point (and with device=True through the device one first: size query, a buffer one
        byte short, the write, all against the same expectations). Returns (messages, status)."""
        nf, tab = self.nf, self.tab
        n = len(recs)
        rows = K.resolve(recs, entries) if entries is not None else None
        own = None
        if entries is not None and strings is None:
            own = strings = tab.flp_ipfix_strings(entries)
        want, want_status = R.run(self.ref, recs, NOW, MONO, G.rows(NAMES), EXPORT, present, parts, entries, flags_decoded=self.flags_decoded, only=only)
        if device:
            before = [self.state.get(v6) for v6 in (False, True)]
            dev_out = device_call(nf, tab, self, recs, present, parts, rows, strings, before)
        rc, buf, off, status, sent = tab.flp_ipfix_write(self.state, recs, self.options(), present, parts, rows, strings) if not device else dev_out
        assert rc == nf.OK
        raw = np.asarray(buf).tobytes()
        msgs = [raw[int(off[i]):int(off[i + 1])] for i in range(n)]
        assert list(status) == want_status
        assert sent == sum(1 for s in want_status if s == 0) and int(off[n]) == len(raw) and int(off[0]) == 0
        seq = self.seq
        for i in range(n):
            if want_status[i]:
                assert msgs[i] == b"", i
                continue
            if only is None or i in only:
                assert msgs[i] == want[i], "flow %d:\n got %s\nwant %s" % (i, msgs[i].hex(), want[i].hex())
                hdr, vals = R.decode_data(msgs[i], self.templates)     # by the product's own template
                assert hdr["export_time"] == EXPORT and hdr["domain"] == 1
            assert struct.unpack_from(">HHII", msgs[i], 0)[1::2] == (len(msgs[i]), seq & 0xFFFFFFFF), i
            seq += 1
        self.seq = seq
        self.sent += [m for m in msgs if m]
        self.check_state()
        if own is not None:
            own.close()
        return msgs, want_status


def device_call(nf, tab, pair, recs, present, parts, rows, strings, before):
    """nfagg_flp_ipfix_write_device on device pointers with canaries behind every output: the size query and a buffer one byte
    short (NFAGG_TRUNCATED: nothing written, the state as it was), then the write."""
    import torch
    L = nf._lib
    n = len(recs)
    o, keep = pair.options()
    d_recs = E.dev(recs)
    feat = None
    if present is not None:
        d_present = E.dev(present)
        d_parts = {k: E.dev(v) for k, v in parts.items() if k != "network_events"}
        feat, _ = tab._pb_features(n, d_present.data_ptr(), {k: v.data_ptr() for k, v in d_parts.items()}, device=True)
    d_rows = E.dev(np.ascontiguousarray(rows, dtype=np.uint32)) if rows is not None else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    d_off = torch.full((n + 1 + 4,), -1, dtype=torch.int64, device="cuda")
    d_status = torch.full((n + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    need, sent = C.c_size_t(0), C.c_size_t(0)
    args = (tab._h, pair.state._t, ptr(d_recs), n, C.byref(feat) if feat is not None else None, ptr(d_rows), strings._t if strings is not None else None,
            C.byref(o))
    rc = L.lib.nfagg_flp_ipfix_write_device(*args, None, 0, ptr(d_off), ptr(d_status), C.byref(sent), C.byref(need))
    total = need.value
    assert rc == L.TRUNCATED, L.lib.nfagg_last_error(tab._h)              # the size query
    d_out = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    if total:
        rc = L.lib.nfagg_flp_ipfix_write_device(*args, ptr(d_out), total - 1, ptr(d_off), ptr(d_status), C.byref(sent), C.byref(need))
        torch.cuda.synchronize()
        assert rc == L.TRUNCATED and need.value == total
        assert bool((d_out == 0xAB).all()) and bool((d_off == -1).all()) and bool((d_status == 0xAB).all())
        assert [pair.state.get(v6) for v6 in (False, True)] == before
    rc = L.lib.nfagg_flp_ipfix_write_device(*args, ptr(d_out), total, ptr(d_off), ptr(d_status), C.byref(sent), C.byref(need))
    torch.cuda.synchronize()
    out, off, status = d_out.cpu().numpy(), d_off.cpu().numpy(), d_status.cpu().numpy()
    assert rc == L.OK and need.value == total and (out[total:] == 0xAB).all() and (off[n + 1:] == -1).all() and (status[n:] == 0xAB).all()
    return rc, out[:total], off[:n + 1].astype(np.uint64), status[:n], sent.value


# ---- flows
def neutral(nf, n, etype=0x0800, proto=47):
    """Flows that set no carry group but the addresses: IP, a protocol without ports, ICMP or flags, no bytes, packets or sampling.
    With a non-IP etype they set none at all."""
    r = np.zeros(n, dtype=nf.FLOW_RECORD)
    m, ids = r["metrics"], r["id"]
    m["eth_protocol"], ids["transport_protocol"] = etype, proto
    for f, last in (("src_ip", 1), ("dst_ip", 2)):
        ids[f][:, :12] = np.frombuffer(V4MAP, dtype=np.uint8)
        ids[f][:, 12:] = (10, 0, 0, last)
    m["start_mono_time_ts"], m["end_mono_time_ts"] = 1_000_000, 2_000_000
    m["if_index_first_seen"], m["direction_first_seen"] = 2, 1
    m["src_mac"], m["dst_mac"] = np.frombuffer(bytes.fromhex("020000000001"), dtype=np.uint8), np.frombuffer(bytes.fromhex("020000000002"), dtype=np.uint8)
    return r


def mixed(nf, O, n, seed, pattern=None):
    """G.stream's scrambled records with their feature parts and informer answers; pattern: per flow True for the v6 family."""
    recs = G.stream(nf, O, n, seed)
    m, ids = recs["metrics"], recs["id"]
    if pattern is not None:
        non_ip = m["eth_protocol"] == 0x0806
        m["eth_protocol"] = np.where(pattern, 0x86DD, 0x0800)
        m["eth_protocol"][non_ip & ~pattern] = 0x0806
        v4 = (m["eth_protocol"] != 0x86DD) & (np.arange(n) % 7 != 3)           # every seventh keeps an address that has no To4()
        for f in ("src_ip", "dst_ip"):
            ids[f][v4, :12] = np.frombuffer(V4MAP, dtype=np.uint8)
    present, parts = CG.content_parts(nf, n, seed + 1)
    x = parts["xlat"]                                                          # most translated addresses v4-mapped, so that v4 flows are sent
    fix = np.arange(n) % 5 != 0
    for f in ("saddr", "daddr"):
        x[f][fix, :12] = np.frombuffer(V4MAP, dtype=np.uint8)
    parts = {k: v for k, v in parts.items()}
    return recs, present, parts, KG.entries_for(recs)


PATTERNS = {"alternating": lambda n: np.arange(n) % 2 == 1, "runs of 64": lambda n: (np.arange(n) // 64) % 2 == 1,
            "one v6 flow per wave": lambda n: np.arange(n) % 64 == 17}


@pytest.mark.parametrize("mix", sorted(PATTERNS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1025])
def test_counts_and_family_interleavings(nf, O, tab, n, mix):
    recs, present, parts, entries = mixed(nf, O, n, seed=n + 7, pattern=PATTERNS[mix](n))
    p = Pair(nf, tab)
    try:
        _, st = p.call(recs, present, parts, entries, device=True)
        p.call(recs[::-1].copy(), present[::-1].copy(), {k: v[::-1].copy() for k, v in parts.items()}, entries)      # from the state the first call left
        if n >= 129:
            assert 0 in st and 1 in st
    finally:
        p.close()


ENTRIES = [("10.0.0.1", dict(namespace="shop", name="cart-1", host_ip="192.168.0.1", host_name="node-a")),
           ("10.0.0.2", dict(namespace="bank", name="vault-2", host_ip="192.168.0.2", host_name="node-b"))]


def setter(nf, group, value):
    """One flow that sets `group` (and what the reference sets with it); returns (record, present byte, parts of one flow, entries)."""
    r = neutral(nf, 1)
    m, ids = r["metrics"], r["id"]
    present = np.zeros(1, dtype=np.uint8)
    parts = {k: np.zeros(1, dtype=nf.ROLLUP_KINDS[k]) for k in CG.KINDS}
    entries = []
    if group == "Bytes":
        m["bytes"] = 1000 + value
    elif group == "Packets":
        m["packets"] = 2000 + value
    elif group == "Sampling":
        m["sampling"] = 3 + value
    elif group == "Addr":
        ids["src_ip"][:, 15], ids["dst_ip"][:, 15], ids["transport_protocol"] = 40 + value, 50 + value, 89
    elif group == "Icmp":
        ids["transport_protocol"], ids["icmp_type"], ids["icmp_code"] = 1, 8 + value, 3 + value
    elif group == "Ports":
        ids["transport_protocol"], ids["src_port"], ids["dst_port"] = 17, 5000 + value, 6000 + value
    elif group == "Flags":
        ids["transport_protocol"], m["flags"] = 6, 0x0912 + value
    elif group in ("XlatSrcPort", "XlatDstPort"):
        present[:] = nf.FEAT_XLAT
        x = parts["xlat"]
        x["saddr"][:, :12] = x["daddr"][:, :12] = np.frombuffer(V4MAP, dtype=np.uint8)
        x["saddr"][:, 15], x["daddr"][:, 15] = 7, 8
        x["sport" if group == "XlatSrcPort" else "dport"] = 7000 + value
    elif group == "Rtt":
        present[:] = nf.FEAT_ADDITIONAL
        parts["additional"]["flow_rtt"] = 123_456 + value
    else:                                                              # a Kubernetes string: "SrcNamespace", ..., "DstHostName"
        side, field = group[:3], group[3:]
        info = dict(name="obj-%d" % value)
        if field == "Namespace":
            info["namespace"] = "ns-%d" % value
        if field == "HostName":
            info["host_ip"], info["host_name"] = "192.168.9.9", "host-%d" % value
        entries = [("10.0.0.1" if side == "Src" else "10.0.0.2", info)]
    return r, present, parts, entries


GROUPS = ["Bytes", "Packets", "Sampling", "Addr", "Icmp", "Ports", "Flags", "XlatSrcPort", "XlatDstPort", "Rtt", "SrcNamespace", "SrcName", "DstNamespace",
          "DstName", "SrcHostName", "DstHostName"]


@pytest.mark.parametrize("group", GROUPS)
def test_one_setting_flow_in_every_position(nf, tab, group):
    """The only flow that sets the group sits in lane 0 of the second wave (the flows before it take the state, the later waves and
    the next block take it); then in lane 63; then in no flow of the call, and the state passes through. For the address group the
    other flows are not IP: they fail until the setter comes."""
    base = 0x0806 if group == "Addr" else 0x0800
    p = Pair(nf, tab)
    try:
        for value, (n, at) in enumerate([(1024 + 70, 64), (130, 127), (70, None)]):
            recs = neutral(nf, n, base)
            present = np.zeros(n, dtype=np.uint8)
            parts = {k: np.zeros(n, dtype=nf.ROLLUP_KINDS[k]) for k in CG.KINDS}
            entries = []
            if at is not None:
                r1, p1, parts1, entries = setter(nf, group, value)
                recs[at], present[at] = r1[0], p1[0]
                for k in parts:
                    parts[k][at] = parts1[k][0]
                if entries:                                        # only the setter's addresses have rows
                    recs["id"]["src_ip"][:, 15], recs["id"]["dst_ip"][:, 15] = 101, 102
                    recs["id"]["src_ip"][at, 15], recs["id"]["dst_ip"][at, 15] = 1, 2
            only = set(range(0, n, 61)) | {at or 0, (at or 0) + 1, max((at or 0) - 1, 0), 1023, 1024, n - 1}
            msgs, st = p.call(recs, present, parts, entries, only={i for i in only if i < n})
            if group == "Addr" and value == 0:
                assert st[:at] == [1] * at and st[at:] == [0] * (n - at)
    finally:
        p.close()


def test_split_invariance(nf, O, tab):
    """A few thousand mixed flows in one call, and in calls cut at fixed and at seeded random positions: the same messages."""
    n = 3000
    recs, present, parts, entries = mixed(nf, O, n, seed=99, pattern=np.random.default_rng(5).integers(0, 3, n) == 0)
    rng = np.random.default_rng(11)
    cuts_list = [[], [1, 64, 65, 1024, 2047], sorted(rng.choice(np.arange(1, n), 9, replace=False).tolist())]
    results = []
    with tab.flp_ipfix_strings(entries) as strings:
        for k, cuts in enumerate(cuts_list):
            p = Pair(nf, tab)
            try:
                bounds = [0] + cuts + [n]
                for a, b in zip(bounds, bounds[1:]):
                    # the restatement is run on the whole-call pass and on sampled flows of the cut passes
                    p.call(recs[a:b], present[a:b], {q: v[a:b] for q, v in parts.items()}, entries, strings,
                           only=None if k == 0 else set(range(0, b - a, 37)))
                results.append(p.sent)
            finally:
                p.close()
    assert results[0] == results[1] == results[2] and len(results[0]) > n // 2


@pytest.mark.parametrize("ln", [0, 1, 254, 255, 256, 1024])
def test_string_lengths_in_each_position_then_carried_from_the_state(nf, tab, ln):
    """Strings of one length in all six positions (distinct text in each), then the table is destroyed and a flow without rows
    carries them out of the state's own bytes."""
    text = lambda c: (bytes([c]) + bytes(range(256)) * 5)[:ln]  # noqa: E731
    entries = [("10.0.0.1", dict(namespace=text(65), name=text(66), host_ip="h", host_name=text(67))),
               ("10.0.0.2", dict(namespace=text(68), name=text(69), host_ip="h", host_name=text(70)))]
    p = Pair(nf, tab)
    try:
        strings = tab.flp_ipfix_strings(entries)
        msgs, st = p.call(neutral(nf, 3), entries=entries, strings=strings)
        strings.close()
        assert st == [0, 0, 0] and len(msgs[0]) >= 6 * ln
        far = neutral(nf, 66)
        far["id"]["src_ip"][:, 15], far["id"]["dst_ip"][:, 15] = 201, 202
        msgs2, st2 = p.call(far, entries=[])
        assert st2 == [0] * 66 and len(msgs2[65]) == len(msgs[0])
        got = p.state.get(False)
        assert got["sourcePodName"] == text(66) and got["destinationNodeName"] == (text(70) if ln else b"")
    finally:
        p.close()


def test_message_of_exactly_max_msg_size_and_one_byte_more(nf, tab):
    entries = [("10.0.0.1", dict(namespace="n" * 300, name="p" * 100))]
    probe = Pair(nf, tab)
    try:
        msgs, _ = probe.call(neutral(nf, 1), entries=entries)
        size = len(msgs[0])
    finally:
        probe.close()
    assert size > 512
    for limit, want in ((size, [0, 0]), (size - 1, [2, 2])):
        p = Pair(nf, tab, max_msg=limit)
        try:
            assert p.call(neutral(nf, 2), entries=entries)[1] == want
            assert p.seq == (2 if limit == size else 0)
            assert p.state.get(False)["sourcePodNamespace"] == b"n" * 300          # the setters ran before the failure
        finally:
            p.close()


def test_a_failed_flows_state_shows_in_the_next_flow_and_the_sequence_stays(nf, tab):
    recs = neutral(nf, 4)
    present = np.zeros(4, dtype=np.uint8)
    parts = {k: np.zeros(4, dtype=nf.ROLLUP_KINDS[k]) for k in CG.KINDS}
    recs["metrics"]["bytes"][1] = 99
    present[1] = nf.FEAT_XLAT                                         # a translated address that has no To4(): flow 1 fails
    parts["xlat"]["saddr"][1, 0], parts["xlat"]["daddr"][1, :12], parts["xlat"]["daddr"][1, 15] = 0x20, np.frombuffer(V4MAP, dtype=np.uint8), 9
    p = Pair(nf, tab)
    try:
        msgs, st = p.call(recs, present, parts, device=True)
        assert st == [0, 1, 0, 0]
        templates = p.templates
        seqs = [R.decode_data(m, templates)[0]["seq"] for m in msgs if m]
        assert seqs == [0, 1, 2]
        octets = [dict(((e, x), v) for e, x, v in R.decode_data(m, templates)[1])[(1, 0)] for m in msgs if m]
        assert octets == [struct.pack(">Q", 0), struct.pack(">Q", 99), struct.pack(">Q", 99)]
    finally:
        p.close()


def test_first_flows_of_the_v4_family_that_are_not_ip_fail_until_an_ip_flow_comes(nf, tab):
    recs = neutral(nf, 70, 0x0806)
    recs["metrics"]["eth_protocol"][66] = 0x0800
    six = neutral(nf, 1, 0x86DD)
    recs[3] = six[0]                                                  # a v6 flow in between sets nothing of the v4 family
    p = Pair(nf, tab)
    try:
        assert p.call(recs)[1] == [1, 1, 1, 0] + [1] * 62 + [0] * 4
    finally:
        p.close()


def test_address_family_failures(nf, tab):
    recs = neutral(nf, 6)
    present = np.zeros(6, dtype=np.uint8)
    parts = {k: np.zeros(6, dtype=nf.ROLLUP_KINDS[k]) for k in CG.KINDS}
    recs["id"]["src_ip"][1, 0] = 0x20                                 # Etype 0x0800 with an address that is not v4-mapped
    recs["id"]["src_ip"][2] = recs["id"]["src_ip"][0]                 # flow 2 sets a mapped one again
    x = parts["xlat"]
    x["saddr"][:, :12] = x["daddr"][:, :12] = np.frombuffer(V4MAP, dtype=np.uint8)
    x["saddr"][:, 15], x["daddr"][:, 15] = 1, 2
    present[3] = present[4] = present[5] = nf.FEAT_XLAT
    x["daddr"][4, 3] = 0x77                                           # v4 family, translated address not mapped
    recs["metrics"]["eth_protocol"][5] = 0x86DD                       # v6 family: any translated address is sent
    x["saddr"][5, 3] = 0x77
    p = Pair(nf, tab)
    try:
        assert p.call(recs, present, parts, device=True)[1] == [0, 1, 0, 0, 1, 0]
    finally:
        p.close()


def test_sampling_probability_is_the_correctly_rounded_quotient(nf, tab):
    rng = np.random.default_rng(3)
    intervals = [1, 2, 3, 7, 10, 2**31, 2**32 - 1] + rng.integers(1, 2**32, 300).tolist()
    recs = neutral(nf, len(intervals))
    recs["metrics"]["sampling"] = intervals
    p = Pair(nf, tab, enterprise=0)
    try:
        msgs, st = p.call(recs)
        assert st == [0] * len(intervals)
        for x, m in zip(intervals, msgs):
            assert m[-8:] == struct.pack(">d", 1.0 / float(x)) and m[-10:-8] == b"\x00\x04", x       # samplingProbability is the last element
    finally:
        p.close()


def test_without_an_enterprise_id_the_nine_elements_are_gone(nf, O, tab):
    recs, present, parts, entries = mixed(nf, O, 200, seed=5, pattern=np.arange(200) % 3 == 0)
    p = Pair(nf, tab, enterprise=0)
    q = Pair(nf, tab, enterprise=2)
    try:
        a, st = p.call(recs, present, parts, entries)
        b, _ = q.call(recs, present, parts, entries)
        assert all(len(x) < len(y) and x[20:] == y[20:20 + len(x) - 20] for x, y, s in zip(a, b, st) if s == 0)
        assert p.state.get(False)["sourcePodName"] == b"" and p.state.get(True)["rtt_ns"] == 0
    finally:
        p.close()
        q.close()


def test_decoded_flags_keep_the_eleven_known_bits(nf, tab):
    recs = neutral(nf, 5, proto=6)
    recs["metrics"]["flags"] = [0xFFFF, 0x0812, 0x0800, 0x07FF, 0]
    for decoded in (False, True):
        p = Pair(nf, tab, flags_decoded=decoded)
        try:
            p.call(recs)
            assert p.state.get(False)["flags"] == 0
        finally:
            p.close()


def test_truncated_host_call_leaves_state_and_outputs(nf, O, tab):
    recs, present, parts, entries = mixed(nf, O, 100, seed=2, pattern=np.arange(100) % 2 == 0)
    p = Pair(nf, tab)
    try:
        p.call(recs[:50], present[:50], {k: v[:50] for k, v in parts.items()}, entries)
        before = [p.state.get(v6) for v6 in (False, True)]
        with tab.flp_ipfix_strings(entries) as strings:
            rows = K.resolve(recs[50:], entries)
            args = (p.state, recs[50:], p.options(), present[50:], {k: v[50:] for k, v in parts.items()}, rows, strings)
            rc, buf, off, status, sent = tab.flp_ipfix_write(*args, out_cap=16)
            assert rc == nf.TRUNCATED and len(buf) == 0 and not status.any() and int(off[-1]) > 16 and not off[:-1].any()
            assert [p.state.get(v6) for v6 in (False, True)] == before
            full = tab.flp_ipfix_write(*args)
            p.state.reset()
            assert p.state.get(False)["src_addr"] is None and p.state.get(True)["bytes"] == 0
        assert full[0] == nf.OK and int(full[2][-1]) == int(off[-1]) and full[4] == sent
    finally:
        p.close()


def test_rows_of_k8s_resolve_index_the_strings_table(nf, O, tab):
    recs, present, parts, entries = mixed(nf, O, 300, seed=21, pattern=np.arange(300) % 4 == 0)
    with nf.K8sTable(entries, None, tab) as k8s:
        rows = tab.k8s_resolve(k8s, recs)
    assert np.asarray(rows).reshape(-1, 2).tolist() == K.resolve(recs, entries).tolist()


def test_python_write_ipfix_over_three_evictions(nf, O, tab):
    got, want = [], []
    ref = R.WriteIpfix(want.append, 2, 512, export_time=EXPORT)
    recs, present, parts, entries = mixed(nf, O, 180, seed=31, pattern=np.arange(180) % 3 == 1)
    with tab.flp_ipfix_strings(entries) as strings:
        w = nf.WriteIpfix(tab, dict(targetHost="collector", targetPort=4739, transport="udp", enterpriseId=2, tplSendInterval="10s"), got.append,
                          strings=strings, names=G.table(nf, NAMES), now_s=EXPORT)
        try:
            assert got == want and len(got) == 2                     # the templates first
            for k, now_s in enumerate((EXPORT, EXPORT + 3, EXPORT + 14)):
                a, b = 60 * k, 60 * (k + 1)
                if now_s - EXPORT >= 10:
                    ref.send_templates(now_s)                         # the refresh interval has passed on the writer's clock
                _, st = R.run(ref, recs[a:b], NOW, MONO, G.rows(NAMES), now_s, present[a:b], {q: v[a:b] for q, v in parts.items()}, entries)
                sent = w.Write(recs[a:b], NOW, MONO, now_s, present[a:b], {q: v[a:b] for q, v in parts.items()}, K.resolve(recs[a:b], entries))
                assert w.failed == [(i, s) for i, s in enumerate(st) if s] and sent == st.count(0)
                assert got == want
            assert w.seqNumber == ref.seq and len(got) == 4 + w.seqNumber      # the templates twice, then one message per sent flow
        finally:
            w.close()


def test_the_pipeline_ends_in_write_ipfix(nf, O, tab):
    got, want = [], []
    ref = R.WriteIpfix(want.append, 2, 65535, export_time=0)
    recs, _, _, entries = mixed(nf, O, 90, seed=41, pattern=np.arange(90) % 2 == 0)
    import io
    with tab.flp_ipfix_strings(entries) as strings, nf.K8sTable(entries, None, tab) as k8s, tab.tls_names() as tls:
        w = nf.WriteIpfix(tab, dict(targetHost="c", targetPort=1, enterpriseId=2), got.append, strings=strings, names=G.table(nf, NAMES))
        try:
            exp = nf.DirectFLPJSON(tab, io.BytesIO(), names=G.table(nf, NAMES), tls_names=tls, k8s=k8s, ipfix=w)
            assert exp.ExportEvicted(recs, NOW, MONO) == 90
            _, st = R.run(ref, recs, NOW, MONO, G.rows(NAMES), NOW // 10**9, None, None, entries)
            assert got == want and exp.ipfix_failed == [(i, s) for i, s in enumerate(st) if s]
        finally:
            w.close()


def test_a_call_that_crosses_the_second_level_of_the_block_scan(nf, O, tab):
    """2^17 + 1 flows: 129 blocks, more than one per thread of the scan over blocks. The stream tiles 512 distinct flows; the
    restatement runs its setters and checks on every flow and builds the bytes of a sample."""
    n = (1 << 17) + 1
    r0, p0, parts0, entries = mixed(nf, O, 512, seed=77, pattern=np.arange(512) % 5 == 2)
    idx = np.random.default_rng(8).integers(0, 512, n)
    idx[1000:70000] = idx[1000:70000] % 3 + 40                        # long stretches in which most groups are set by no flow
    recs, present, parts = r0[idx], p0[idx], {k: v[idx] for k, v in parts0.items()}
    only = set(range(0, n, 4099)) | {1023, 1024, 1025, 65535, 65536, 69999, 70000, 70001, n - 2, n - 1}
    p = Pair(nf, tab)
    try:
        p.call(recs, present, parts, entries, only=only)
    finally:
        p.close()
