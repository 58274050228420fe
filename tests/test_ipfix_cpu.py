"""IPFIX export, CPU side: the template messages of nfagg_ipfix_template against literals written out from ipfix.go's field
lists, the argument checks the encode entry points make before any device work, the restatement of tests/ipfix_ref.py
against hand-written messages, and the bookkeeping of pipeline.IPFIX (templates first, sequence numbers, the UDP
template refresh) with the GPU encode replaced by the restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ipfix_ref as R  # noqa: E402

# 16-byte header | set 2, length 84 | template id, 19 fields | (id, length) x 19
V4_TEMPLATE = bytes.fromhex(
    "000a 0064 01020304 00000005 00000001"
    "0002 0054" "0100 0013"
    "0100 0002" "003d 0001" "0038 0006" "0050 0006" "0008 0004" "000c 0004" "0004 0001" "0007 0002" "000b 0002" "00b0 0001" "00b1 0001"
    "0001 0008" "0006 0002" "0096 0004" "0098 0008" "0097 0004" "0099 0008" "0002 0008" "0052 ffff")
V6_TEMPLATE = bytes.fromhex(
    "000a 0064 01020304 00000005 00000001"
    "0002 0054" "0101 0013"
    "0100 0002" "003d 0001" "0038 0006" "0050 0006" "001b 0010" "001c 0010" "00c1 0001" "0007 0002" "000b 0002" "00b2 0001" "00b3 0001"
    "0001 0008" "0006 0002" "0096 0004" "0098 0008" "0097 0004" "0099 0008" "0002 0008" "0052 ffff")


def test_template_messages_are_the_literals(nf):
    assert len(V4_TEMPLATE) == len(V6_TEMPLATE) == 100
    assert nf.ipfix_template(False, 0x01020304, 5) == V4_TEMPLATE
    assert nf.ipfix_template(True, 0x01020304, 5) == V6_TEMPLATE
    assert R.template_message(False, 0x01020304, 5) == V4_TEMPLATE and R.template_message(True, 0x01020304, 5) == V6_TEMPLATE
    col = R.Collector()
    for msg, tid, fields in ((V4_TEMPLATE, 256, R.FIELDS_V4), (V6_TEMPLATE, 257, R.FIELDS_V6)):
        d = col.decode(msg)
        assert (d["kind"], d["template_id"], d["seq"], d["export_time"], d["domain"], d["set_len"]) == ("template", tid, 5, 0x01020304, 1, 84)
        assert [R.REGISTRY[i][0] for i, _ in d["fields"]] == fields
    assert set(col.templates) == {(1, 256), (1, 257)}
    # another domain and other template ids go where the options say
    t = nf.ipfix_template(True, 0, 0xFFFFFFFF, obs_domain_id=7, template_ids=(300, 301))
    assert t[8:16] == bytes.fromhex("ffffffff 00000007") and t[20:22] == bytes.fromhex("012d")


def test_template_argument_checks(nf):
    L = nf._lib
    o, _ = nf.ipfix_options(export_time_s=1, seq0=2)
    buf = (C.c_uint8 * 128)(*([0xAB] * 128))
    n = C.c_size_t(0)
    assert L.lib.nfagg_ipfix_template(None, 0, buf, 128, C.byref(n)) == L.EINVAL
    assert L.lib.nfagg_ipfix_template(C.byref(o), 0, buf, 128, None) == L.EINVAL
    assert L.lib.nfagg_ipfix_template(C.byref(o), 0, buf, 99, C.byref(n)) == L.TRUNCATED and n.value == 100
    assert bytes(buf) == b"\xab" * 128, "a truncated call writes nothing"
    assert L.lib.nfagg_ipfix_template(C.byref(o), 0, None, 0, C.byref(n)) == L.TRUNCATED and n.value == 100
    o.struct_size -= 4
    assert L.lib.nfagg_ipfix_template(C.byref(o), 0, buf, 128, C.byref(n)) == L.EINVAL
    assert b"struct_size" in L.lib.nfagg_last_error(None)


@pytest.mark.parametrize("device", [False, True])
def test_encode_rejects_bad_options_before_device_work(nf, device):
    """Checked before the handle: no GPU is needed to see these refused."""
    L = nf._lib
    fn = L.lib.nfagg_encode_ipfix_device if device else L.lib.nfagg_encode_ipfix
    off = np.zeros(2, dtype=np.uint64)
    need = C.c_size_t(0)
    rec = np.zeros(1, dtype=nf.FLOW_RECORD)

    def call(o):
        return fn(None, rec.ctypes.data_as(C.c_void_p), 1, C.byref(o) if o is not None else None, None, 0,
                  off.ctypes.data_as(C.c_void_p), C.byref(need))

    assert call(None) == L.EINVAL and b"null options" in L.lib.nfagg_last_error(None)
    o, keep = nf.ipfix_options(names=nf.intf_table([(1, None, "lo", "")]))
    o.struct_size += 8
    assert call(o) == L.EINVAL and b"struct_size" in L.lib.nfagg_last_error(None)
    bad = nf.intf_table([(1, None, "lo", ""), (2, None, "eth0", "")])
    bad[1]["name_len"] = 17
    o, keep = nf.ipfix_options(names=bad)
    assert call(o) == L.EINVAL and b"row 1: name too long" in L.lib.nfagg_last_error(None)
    o, keep = nf.ipfix_options(unknown=b"u" * 16)
    o.unknown_len = 17
    assert call(o) == L.EINVAL and b"namer table" in L.lib.nfagg_last_error(None)
    o, keep = nf.ipfix_options()
    o.n_names = 3                                     # rows promised, no table
    assert call(o) == L.EINVAL and b"namer table" in L.lib.nfagg_last_error(None)
    o, keep = nf.ipfix_options()
    assert call(o) == L.EINVAL and b"null argument" in L.lib.nfagg_last_error(None)     # good options, no handle


# ---- the restatement against hand-written messages

NOW, MONO = 1_700_000_000_123_456_789, 10_000_000_000
NAMES = [(2, None, b"eth0"), (2, bytes.fromhex("020000000001"), b"eth0-mac"), (3, None, b"veth3"), (6, None, b""),
         (8, None, b"x" * 16)]


def _rec(nf, src, dst, sport, dport, proto, eth, direction, if_index, start, end, nbytes=0, packets=0, flags=0,
         smac="020000000001", dmac="0a0b0c0d0e0f", icmp=(0, 0)):
    r = np.zeros(1, dtype=nf.FLOW_RECORD)
    r["id"]["src_ip"] = np.frombuffer(src, dtype=np.uint8)
    r["id"]["dst_ip"] = np.frombuffer(dst, dtype=np.uint8)
    r["id"]["src_port"], r["id"]["dst_port"], r["id"]["transport_protocol"] = sport, dport, proto
    r["id"]["icmp_type"], r["id"]["icmp_code"] = icmp
    m = r["metrics"]
    m["start_mono_time_ts"], m["end_mono_time_ts"], m["bytes"], m["packets"] = start, end, nbytes, packets
    m["eth_protocol"], m["flags"], m["direction_first_seen"], m["if_index_first_seen"] = eth, flags, direction, if_index
    m["src_mac"] = np.frombuffer(bytes.fromhex(smac), dtype=np.uint8)
    m["dst_mac"] = np.frombuffer(bytes.fromhex(dmac), dtype=np.uint8)
    return r


V4MAP = bytes(10) + b"\xff\xff"
SIX1, SIX2 = bytes.fromhex("20010db8000000000000000000000001"), bytes.fromhex("20010db8000000000000000000000002")


def test_restatement_v4_flow(nf):
    r = _rec(nf, V4MAP + bytes([10, 0, 0, 1]), V4MAP + bytes([192, 168, 1, 2]), 443, 51234, 6, 0x0800, 1, 2,
             MONO - 2_500_000_000, MONO - 500_000_000, 123456789, 1000, 0x12)
    want = bytes.fromhex(
        "000a 0065 6553f100 00000029 00000001"       # version 10, length 101, export time 1700000000, seq 41, domain 1
        "0100 0055"                                  # set: template 256, 101 - 16
        "0800" "01" "020000000001" "0a0b0c0d0e0f"    # ethernetType, flowDirection, MACs
        "0a000001" "c0a80102" "06" "01bb" "c822" "00" "00"
        "00000000075bcd15" "0012"                    # octets, tcpControlBits
        "6553f0fd" "0000018bcfe55eb7"                # start: now - 2.5 s = 1699999997.623456789
        "6553f0ff" "0000018bcfe56687"                # end:   now - 0.5 s
        "00000000000003e8"                           # packets
        "08" + b"eth0-mac".hex())                    # egress: lMAC = src_mac, the exact (index, MAC) row
    buf, off = R.encode(r, NOW, MONO, NAMES, 1_700_000_000, 41)
    assert buf == want and off.tolist() == [0, 101]
    d = R.Collector()
    d.decode(V4_TEMPLATE)
    rec = d.decode(buf)["records"][0]
    assert rec["sourceIPv4Address"] == bytes([10, 0, 0, 1]) and rec["interfaceName"] == "eth0-mac"
    assert rec["flowStartMilliseconds"] == 1699999997623 and rec["sourceTransportPort"] == 443


def test_restatement_v6_flow(nf):
    r = _rec(nf, SIX1, SIX2, 53, 40000, 17, 0x86DD, 0, 3, MONO, MONO, 77, 1)
    want = bytes.fromhex(
        "000a 007a 6553f100 00000000 00000001"       # length 117 + 5
        "0101 006a"
        "86dd" "00" "020000000001" "0a0b0c0d0e0f" + SIX1.hex() + SIX2.hex() +
        "11" "0035" "9c40" "00" "00"
        "000000000000004d" "0000"
        "6553f100" "0000018bcfe5687b" "6553f100" "0000018bcfe5687b"
        "0000000000000001"
        "05" + b"veth3".hex())
    buf, off = R.encode(r, NOW, MONO, NAMES, 1_700_000_000, 0)
    assert buf == want and off.tolist() == [0, 122]


def test_restatement_unmapped_addresses_empty_long_and_unknown_names(nf):
    t = (MONO, MONO)
    tail = "00" "00" "0000000000000000" "0000" "6553f100 0000018bcfe5687b 6553f100 0000018bcfe5687b" "0000000000000000"
    cases = [   # (eth, if_index, name bytes): v4 template with 2001:db8:: addresses -> 0.0.0.0 (eth 0 is v4 too)
        (0x0000, 99, b"unknown"), (0x0800, 6, b""), (0x0800, 8, b"x" * 16)]
    for eth, ifx, name in cases:
        r = _rec(nf, SIX1, SIX2, 1, 2, 6, eth, 0, ifx, *t)
        ln = 93 + len(name)
        want = bytes.fromhex(
            "000a %04x 00000001 00000007 00000001" % ln + "0100 %04x" % (ln - 16) +
            "%04x" % eth + "00" "020000000001" "0a0b0c0d0e0f" "00000000" "00000000" "06" "0001" "0002" + tail +
            "%02x" % len(name) + name.hex())
        buf, off = R.encode(r, NOW, MONO, NAMES, 1, 7)
        assert buf == want, (eth, ifx)
    # a custom unknown name
    buf, _ = R.encode(_rec(nf, SIX1, SIX2, 1, 2, 6, 0x0800, 0, 99, *t), NOW, MONO, NAMES, 1, 7, unknown=b"?")
    assert buf[-2:] == b"\x01?"


def test_restatement_times_before_1970(nf):
    # now = 1 s after the epoch; the flow started 3.5 s before now: t = -2.5 s -> Unix() = -3, UnixMilli() = -2500
    r = _rec(nf, V4MAP + bytes(4), V4MAP + bytes(4), 0, 0, 1, 0x0800, 0, 2, MONO - 3_500_000_000, MONO, icmp=(8, 0))
    buf, _ = R.encode(r, 1_000_000_000, MONO, NAMES, 1, 0)
    assert buf[48:50] == b"\x08\x00"
    assert buf[60:64] == bytes.fromhex("fffffffd") and buf[64:72] == bytes.fromhex("fffffffffffff63c")
    assert buf[72:76] == bytes.fromhex("00000001") and buf[76:84] == bytes.fromhex("00000000000003e8")


def test_restatement_sequence_wraps(nf):
    r = np.concatenate([_rec(nf, V4MAP + bytes([1, 2, 3, k]), V4MAP + bytes(4), k, 0, 6, 0x0800, 0, 2, MONO, MONO) for k in range(20)])
    buf, off = R.encode(r, NOW, MONO, NAMES, 5, 0xFFFFFFF0)
    assert len(off) == 21 and all(int(off[i + 1]) - int(off[i]) == 97 for i in range(20))
    seqs = [buf[int(off[i]) + 8:int(off[i]) + 12] for i in range(20)]
    assert seqs[0] == bytes.fromhex("fffffff0") and seqs[15] == bytes.fromhex("ffffffff")
    assert seqs[16] == bytes.fromhex("00000000") and seqs[19] == bytes.fromhex("00000003")


def test_decoder_variable_length_escape():
    """The 255 escape of getFieldLength (a name never needs it: at most 16 bytes) in the decoder alone."""
    col = R.Collector()
    col.decode(V4_TEMPLATE)
    body = bytes(72) + b"\xff\x01\x00" + b"n" * 256
    msg = R.header(16 + 4 + len(body), 0, 0, 1) + bytes.fromhex("0100%04x" % (4 + len(body))) + body
    assert col.decode(msg)["records"][0]["interfaceName"] == "n" * 256
    with pytest.raises(ValueError):
        col.decode(R.header(20 + 73, 0, 0, 1) + bytes.fromhex("0101%04x" % 77) + bytes(73))   # v6 data, short


# ---- pipeline.IPFIX bookkeeping, the GPU encode replaced by the restatement

class FakeClock:
    def __init__(self, t):
        self.t = t

    def __call__(self):
        return self.t


def _exporter(nf, transport, clock, sent):
    def encode(raw, now_ns, mono_ns, names, export_time_s, seq0, unknown, obs_domain_id):
        buf, off = R.encode(raw, now_ns, mono_ns, NAMES, export_time_s, seq0, unknown, obs_domain_id)
        return np.frombuffer(buf, dtype=np.uint8), off
    return nf.StartIPFIXExporter(None, lambda m: sent.append(bytes(m)), transport, clock=clock, mono_clock=lambda: MONO, encode=encode)


def _flows(nf, n, base=0):
    if n == 0:
        return np.zeros(0, dtype=nf.FLOW_RECORD)
    return np.concatenate([_rec(nf, V4MAP + bytes([10, 0, (base + k) >> 8, (base + k) & 255]), V4MAP + bytes(4), 1000 + k, 80, 6,
                                0x86DD if k % 3 == 0 else 0x0800, 0, 2, MONO, MONO) for k in range(n)])


@pytest.mark.parametrize("transport", ["udp", "tcp"])
def test_exporter_templates_first_then_one_message_per_flow(nf, transport):
    clock, sent = FakeClock(NOW), []
    ipf = _exporter(nf, transport, clock, sent)
    assert sent == [R.template_message(False, 1_700_000_000, 0), R.template_message(True, 1_700_000_000, 0)]
    assert ipf.ExportEvicted(_flows(nf, 5), NOW, MONO) == 5 and ipf.seqNumber == 5
    assert ipf.ExportEvicted(_flows(nf, 0), NOW, MONO) == 0 and ipf.seqNumber == 5
    assert ipf.ExportEvicted(_flows(nf, 3, 5), NOW, MONO) == 3 and ipf.seqNumber == 8
    assert len(sent) == 2 + 8
    col = R.Collector()
    for m in sent[:2]:
        col.decode(m)
    for k, m in enumerate(sent[2:]):
        d = col.decode(m)
        kl = k if k < 5 else k - 5                   # index inside its eviction
        assert d["seq"] == k and d["set_id"] == (257 if kl % 3 == 0 else 256)
        assert d["records"][0]["sourceTransportPort"] == 1000 + kl


def test_exporter_udp_refreshes_templates_after_a_second(nf):
    clock, sent = FakeClock(NOW), []
    ipf = _exporter(nf, "udp", clock, sent)
    ipf.ExportEvicted(_flows(nf, 2), NOW, MONO)
    assert len(sent) == 4
    clock.t += 999_999_999                           # not yet 1 s since the templates
    ipf.ExportEvicted(_flows(nf, 1), NOW, MONO)
    assert len(sent) == 5
    clock.t += 1                                     # 1 s: both templates, v4 then v6, before the next data message
    ipf.ExportEvicted(_flows(nf, 2), NOW, MONO)
    assert len(sent) == 9
    assert sent[5] == R.template_message(False, 1_700_000_001, 3) and sent[6] == R.template_message(True, 1_700_000_001, 3)
    col = R.Collector()
    col.decode(sent[5])
    col.decode(sent[6])
    assert [col.decode(m)["seq"] for m in sent[7:]] == [3, 4]
    clock.t += 5_000_000_000
    ipf.ExportEvicted(_flows(nf, 0), NOW, MONO)      # nothing to send: no refresh either
    assert len(sent) == 9


def test_exporter_udp_refresh_inside_a_batch(nf):
    """The clock passes 1 s while one eviction's messages go out: the templates go in before the next data message,
    with the sequence number of the data records sent so far."""
    t = FakeClock(NOW)
    sent = []

    def send(m):
        sent.append(bytes(m))
        t.t += 300_000_000                           # every send takes 0.3 s

    def encode(raw, now_ns, mono_ns, names, export_time_s, seq0, unknown, obs_domain_id):
        buf, off = R.encode(raw, now_ns, mono_ns, NAMES, export_time_s, seq0, unknown, obs_domain_id)
        return np.frombuffer(buf, dtype=np.uint8), off

    ipf = nf.StartIPFIXExporter(None, send, "udp", clock=t, encode=encode)   # templates sent from +0.0 s
    ipf.ExportEvicted(_flows(nf, 4), NOW, MONO)                             # data at +0.6, +0.9; at +1.2 s the refresh
    kinds = ["template" if m[16:18] == b"\x00\x02" else "data" for m in sent]
    assert kinds == ["template", "template", "data", "data", "template", "template", "data", "data"]
    assert sent[4] == R.template_message(False, 1_700_000_001, 2) and sent[5] == R.template_message(True, 1_700_000_001, 2)
    assert [m[8:12] for m in sent[6:]] == [(2).to_bytes(4, "big"), (3).to_bytes(4, "big")]


def test_exporter_tcp_never_refreshes(nf):
    clock, sent = FakeClock(NOW), []
    ipf = _exporter(nf, "tcp", clock, sent)
    for k in range(3):
        clock.t += 10_000_000_000
        ipf.ExportEvicted(_flows(nf, 2), NOW, MONO)
    assert len(sent) == 2 + 6 and ipf.seqNumber == 6


def test_exporter_export_flows_until_close(nf):
    import queue
    clock, sent = FakeClock(NOW), []
    ipf = _exporter(nf, "tcp", clock, sent)
    q = queue.Queue()
    q.put((_flows(nf, 3), NOW, MONO))
    q.put((_flows(nf, 2), NOW, MONO))
    q.put(nf.CLOSE)
    ipf.ExportFlows(q)
    assert len(sent) == 7 and ipf.seqNumber == 5
    with pytest.raises(ValueError):
        nf.IPFIX(None, print, "sctp", encode=lambda *a: None)


def test_c_driver_builds_against_the_header_alone(nf, tmp_path):
    """tools/c/nfagg_ipfix_cdriver.c: plain C11 with -Werror, linked against lib/libnfagg.so alone (what a cgo shim sees)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "netobserv-ebpf-agent_amd", "lib")
    exe = str(tmp_path / "nfagg_ipfix_cdriver")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tools", "c", "nfagg_ipfix_cdriver.c"), "-o", exe, "-L", libdir, "-lnfagg", "-Wl,-rpath," + libdir])
    needed = subprocess.check_output(["readelf", "-d", exe], text=True)
    assert "libnfagg.so" in needed and "torch" not in needed and "python" not in needed


def test_flow_times_on_the_edges_against_python_integers():
    """ipfix_ref.flow_times on the edges of tests/test_export_edges_gpu.py: time stamps ahead of the clock by a wrap, 2^63 away
    from it, zero; clocks before 1970. Expected: now.Add(-Duration(mono - ts)) with the subtraction and the negation wrapping
    in int64 (record.go:90-97), then uint32(t.Unix()) and uint64(t.UnixMilli()) (ipfix.go:286-300), both flooring."""
    mono = 2_500_000
    ts = [0, 1, mono - 1, mono, mono + 1, 2**64 - 5, 2**64 - 1, 2**63 + 12345, 2**63, 2**63 - 1, (mono + 2**63) % 2**64, (mono + 2**63 + 1) % 2**64,
          (mono - 2**63 + 1) % 2**64, mono - 999_999, mono - 1_000_000, 123_456_789_012_345_678]
    for now in (1_700_000_000_123_456_789, 5, 0, -1, -999_999, -10**9, -10**15, -10**17, 2**32 * 10**9 - 1, 2**32 * 10**9):
        sec, ms = R.flow_times(np.array(ts, dtype=np.uint64), now, mono)
        for k, v in enumerate(ts):
            delta = (mono - v) % 2**64
            d = -(delta - 2**64 if delta >= 2**63 else delta)
            t = now + (d if d < 2**63 else d - 2**64)
            assert int(sec[k]) == (t // 10**9) & 0xFFFFFFFF, (now, v)
            assert int(ms[k]) == (t // 10**6) % 2**64, (now, v)
