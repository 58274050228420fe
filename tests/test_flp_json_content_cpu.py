"""direct-FLP JSON lines of MapTracer flows, CPU side: the restatement of tests/flp_json_content_ref.py pinned against the
expectations of the reference's own tests (tests/golden/flp_content_vectors.json), against hand-written lines for the
edges of every rule, and its name tables against their sizes and ends; the new entry points' exports, signatures and the
argument checks they make before any device work."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_content_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flp_content_vectors.json")
NOW, MONO, RECEIVED = 1_700_000_000_123_456_789, 10_000_000_000, 1_700_000_000
V4MAP = bytes(10) + b"\xff\xff"
AGENT = V4MAP + bytes([10, 9, 8, 7])

# ---- building a flow's bytes from field values (bpf/types.h layouts)
_ID = struct.Struct("<16s16sHHBBBx")
_METRICS = struct.Struct("<QQQIHH6s6sIIIBBBB6s2x6IHHHBB4x")


def record(src_ip=bytes(16), dst_ip=bytes(16), src_port=0, dst_port=0, transport_protocol=0, icmp_type=0, icmp_code=0, start=0, end=0,
           bytes_=0, packets=0, eth_protocol=0, flags=0, src_mac=bytes(6), dst_mac=bytes(6), if_index=0, sampling=0, direction=0, dscp=0,
           observed=(), ssl_version=0, tls_cipher_suite=0, tls_key_share=0, tls_types=0):
    oi = [ix for ix, _ in observed] + [0] * (6 - len(observed))
    od = bytes(d for _, d in observed) + bytes(6 - len(observed))
    return _ID.pack(src_ip, dst_ip, src_port, dst_port, transport_protocol, icmp_type, icmp_code) + _METRICS.pack(
        start, end, bytes_, packets, eth_protocol, flags, src_mac, dst_mac, if_index, 0, sampling, direction, 0, dscp, len(observed), od,
        *oi, ssl_version, tls_cipher_suite, tls_key_share, tls_types, 0)


def additional(flow_rtt=0, ipsec_encrypted_ret=0, ipsec_encrypted=0):
    return struct.pack("<QQQiHBx", 1, 2, flow_rtt, ipsec_encrypted_ret, 0x0800, ipsec_encrypted)


def dns(latency=0, id=0, flags=0, errno=0, name=b""):
    return struct.pack("<QQQHHHB32sx", 1, 2, latency, id, flags, 0x0800, errno, name)


def drops(bytes=0, packets=0, latest_drop_cause=0, latest_flags=0, latest_state=0):
    return struct.pack("<QQHHIHHB3x", 1, 2, bytes, packets, latest_drop_cause, latest_flags, 0x0800, latest_state)


def xlat(saddr=bytes(16), daddr=bytes(16), sport=0, dport=0, zone_id=0):
    return struct.pack("<QQ16s16sHHHH", 1, 2, saddr, daddr, sport, dport, zone_id, 0x0800)


def quic(version=0, seen_long_hdr=0, seen_short_hdr=0):
    return struct.pack("<QQIHBB", 1, 2, version, 0x0800, seen_long_hdr, seen_short_hdr)


BUILD = {"additional": additional, "dns": dns, "drops": drops, "xlat": xlat, "quic": quic}
BASE = record(eth_protocol=0x0806, if_index=2, start=MONO, end=MONO)
NAMES = [(2, None, b"eth0", b"")]


def content(parts, rec=BASE):
    """The keys the parts add to the line of `rec`, as the text between the base line's keys: {key: JSON value text}."""
    base = R.record_to_map(rec, NOW, MONO, NAMES, AGENT, RECEIVED)
    full = R.add_content(dict(base), parts)
    assert all(full[k] == v for k, v in base.items()), "a part changed a base key"
    return {k.decode(): R.marshal_sorted({b"": v})[4:-1].decode("latin-1") for k, v in full.items() if k not in base}


# ---- the reference's own expectations

def _plain(v):
    if isinstance(v, bytes):
        return v.decode()
    return [_plain(x) for x in v] if isinstance(v, list) else v


def _vectors():
    with open(GOLDEN) as f:
        doc = json.load(f)
    return doc["time_ms"], doc["vectors"]


@pytest.mark.parametrize("k", range(6))
def test_restatement_gives_the_map_the_reference_tests_expect(k):
    time_ms, vectors = _vectors()
    assert len(vectors) == 6
    v = vectors[k]
    ident = dict(v["id"])
    m = dict(v["metrics"])
    names = [(10 + j, None, name.encode(), b"") for j, (name, _) in enumerate(v["interfaces"])]
    rec = record(bytes.fromhex(ident.pop("src_ip")), bytes.fromhex(ident.pop("dst_ip")), start=MONO, end=MONO, bytes_=m.pop("bytes", 0),
                 src_mac=bytes.fromhex(m.pop("src_mac")), dst_mac=bytes.fromhex(m.pop("dst_mac")), if_index=10,
                 direction=v["interfaces"][0][1], observed=[(10 + j, d) for j, (_, d) in enumerate(v["interfaces"])][1:], **ident, **m)
    parts = {}
    for kind, fields in v["parts"].items():
        f = {key: bytes.fromhex(val) if isinstance(val, str) else val for key, val in fields.items()}
        parts[kind] = BUILD[kind](**f)
    got = R.add_content(R.record_to_map(rec, time_ms * 10**6, MONO, names, bytes.fromhex(v["agent_ip"]), RECEIVED), parts)
    got = {key.decode(): _plain(val) for key, val in got.items()}
    assert got.pop("TimeReceived") == RECEIVED                    # the reference reads the clock; its tests do not pin it
    want = {key: val for key, val in v["expected"].items() if key not in v["not_restated"]}
    assert set(v["not_restated"]) <= set(v["expected"]) and not set(v["not_restated"]) & set(got)
    assert got == want


# ---- the edges of every rule, one case each, as the JSON text of the added keys

def test_no_part_and_parts_whose_gating_fields_are_zero_add_nothing_but_quic():
    assert content({}) == {}
    assert content({"dns": dns(latency=5, flags=3, name=b"\x01a"), "drops": drops(bytes=9, packets=9, latest_flags=1, latest_state=1),
                    "xlat": xlat(sport=1, dport=2, zone_id=3), "additional": additional()}) == {}
    assert content({"quic": quic()}) == {"QuicVersion": '"QUIC v1"', "QuicSeenLongHdr": "0", "QuicSeenShortHdr": "0"}


def test_dns_latency_with_the_top_bit_set_is_negative_and_truncates_towards_zero():
    c = content({"dns": dns(latency=2**64 - 1_500_000, id=7)})
    assert c == {"DnsId": "7", "DnsFlags": "0", "DnsFlagsResponseCode": '"NoError"', "DnsLatencyMs": "-1"}
    assert content({"dns": dns(latency=2**63, id=7)})["DnsLatencyMs"] == "-9223372036854"
    assert content({"dns": dns(latency=999_999, id=7)})["DnsLatencyMs"] == "0"
    assert content({"dns": dns(latency=0, id=65535, flags=65535)}) == {
        "DnsId": "65535", "DnsFlags": "65535", "DnsFlagsResponseCode": '"UnDefined"', "DnsLatencyMs": "0"}


def test_dns_id_zero_with_errno_gives_only_the_errno():
    assert content({"dns": dns(latency=10**9, id=0, flags=0x8003, errno=110, name=b"\x03www")}) == {"DnsErrno": "110"}
    assert content({"dns": dns(id=1, errno=255)})["DnsErrno"] == "255"


def test_dns_rcodes_eleven_to_fifteen_are_undefined():
    for rc in range(16):
        want = R.RCODES[rc] if rc <= 10 else "UnDefined"
        assert content({"dns": dns(id=1, flags=0x8180 | rc)})["DnsFlagsResponseCode"] == '"%s"' % want
    assert R.RCODES[3] == "NXDomain" and R.RCODES[10] == "NotZone"


def test_dns_name_is_dotted_then_escaped():
    assert content({"dns": dns(id=1, name=b"\x03www\x07example\x03com")})["DnsName"] == '"www.example.com"'
    c = content({"dns": dns(id=1, name=b'\x04"\\\x01\x80\x02\t\n')})
    assert c["DnsName"].encode("latin-1") == b'"\\"\\\\\\u0001\x80.\\t\\n"'
    # stops: a zero length, a compression pointer, a label that runs past the name; 32 bytes without a NUL
    assert "DnsName" not in content({"dns": dns(id=1, name=b"")})
    assert "DnsName" not in content({"dns": dns(id=1, name=b"\xc0\x0c")})
    assert content({"dns": dns(id=1, name=b"\x01a\xc0\x0c")})["DnsName"] == '"a"'
    assert content({"dns": dns(id=1, name=b"\x01a\x05bc")})["DnsName"] == '"a"'
    assert content({"dns": dns(id=1, name=b"\x1f" + b"x" * 31)})["DnsName"] == '"%s"' % ("x" * 31)
    assert content({"dns": dns(id=1, name=b"\x0fabcdefghijklmno\x0fabcdefghijklmno")})["DnsName"] == '"abcdefghijklmno.abcdefghijklmno"'


def test_drop_causes_known_unknown_ovs_and_network_event():
    def cause(c, **kw):
        return content({"drops": drops(latest_drop_cause=c, **kw)})
    assert cause(2, bytes=65535, packets=1, latest_flags=0x200, latest_state=6) == {
        "PktDropBytes": "65535", "PktDropPackets": "1", "PktDropLatestFlags": "512", "PktDropLatestState": '"TCP_CLOSE"',
        "PktDropLatestDropCause": '"SKB_DROP_REASON_NOT_SPECIFIED"'}
    assert cause(5)["PktDropLatestDropCause"] == '"SKB_DROP_REASON_TCP_CSUM"'
    assert cause(13)["PktDropLatestDropCause"] == '"SKB_DROP_REASON_UNICAST_IN_L2_MULTICAST"'
    assert cause(80)["PktDropLatestDropCause"] == '"SKB_DROP_REASON_TC_RECLASSIFY_LOOP"'
    assert cause((3 << 16) + 1)["PktDropLatestDropCause"] == '"OVS_DROP_LAST_ACTION"'
    assert cause((3 << 16) + 11)["PktDropLatestDropCause"] == '"OVS_DROP_IP_TTL"'
    assert cause(1 << 24)["PktDropLatestDropCause"] == '"NetworkEvent_Unknown"'
    assert cause((1 << 24) + 4)["PktDropLatestDropCause"] == '"NetworkEvent_NetworkPolicy"'
    assert cause((1 << 24) + 9)["PktDropLatestDropCause"] == '"NetworkEvent_UDNIsolation"'
    for unknown in (1, 81, 3 << 16, (3 << 16) + 12, (1 << 24) + 10, (1 << 16) + 5, 2**32 - 1):
        assert cause(unknown)["PktDropLatestDropCause"] == '"SKB_DROP_UNKNOWN_CAUSE"'
    assert [cause(2, latest_state=s)["PktDropLatestState"] for s in (0, 1, 11, 12, 255)] == [
        '"TCP_INVALID_STATE"', '"TCP_ESTABLISHED"', '"TCP_NEW_SYN_RECV"', '"TCP_INVALID_STATE"', '"TCP_INVALID_STATE"']


def test_xlat_needs_both_addresses_and_does_not_look_at_the_ethertype():
    a, b = V4MAP + bytes([1, 2, 3, 4]), bytes.fromhex("20010db8000000000000000000000005")
    assert content({"xlat": xlat(a, b, 1, 2, 100)}) == {
        "ZoneId": "100", "XlatSrcPort": "1", "XlatDstPort": "2", "XlatSrcAddr": '"1.2.3.4"', "XlatDstAddr": '"2001:db8::5"'}
    assert content({"xlat": xlat(a, b, 0, 0, 0)}) == {"ZoneId": "0", "XlatSrcAddr": '"1.2.3.4"', "XlatDstAddr": '"2001:db8::5"'}
    assert content({"xlat": xlat(a, bytes(16), 1, 2, 100)}) == {}               # one address zero: no key at all
    assert content({"xlat": xlat(bytes(16), b, 1, 2, 100)}) == {}
    assert content({"xlat": xlat(a, V4MAP + bytes(4), 1, 2, 100)}) == {}        # net.IPv4zero in its 16-byte form
    assert content({"xlat": xlat(a, bytes(15) + b"\x01", 1, 2, 100)})["XlatDstAddr"] == '"::1"'


def test_ipsec_status_and_negative_return_code_and_rtt():
    assert content({"additional": additional(ipsec_encrypted_ret=-1, ipsec_encrypted=1)}) == {"IPSecRetCode": "-1", "IPSecStatus": '"error"'}
    assert content({"additional": additional(ipsec_encrypted_ret=-2**31)})["IPSecRetCode"] == "-2147483648"
    assert content({"additional": additional(ipsec_encrypted_ret=7)}) == {"IPSecRetCode": "7", "IPSecStatus": '"error"'}
    assert content({"additional": additional(ipsec_encrypted=1)}) == {"IPSecRetCode": "0", "IPSecStatus": '"success"'}
    assert content({"additional": additional(flow_rtt=10_000_000)}) == {"TimeFlowRttNs": "10000000"}
    assert content({"additional": additional(flow_rtt=2**64 - 1)}) == {"TimeFlowRttNs": "-1"}


def test_quic_versions():
    assert content({"quic": quic(1, 1, 255)}) == {"QuicVersion": '"QUIC v2"', "QuicSeenLongHdr": "1", "QuicSeenShortHdr": "255"}
    assert content({"quic": quic(2)})["QuicVersion"] == '"QUIC Unknown (2)"'
    assert content({"quic": quic(0xFFFFFFFF)})["QuicVersion"] == '"QUIC Unknown (4294967295)"'


def test_whole_line_has_the_keys_in_byte_order():
    rec = record(V4MAP + bytes([6, 7, 8, 9]), V4MAP + bytes([10, 11, 12, 13]), 23000, 443, 6, start=MONO, end=MONO, bytes_=456, packets=123,
                 eth_protocol=0x0800, flags=0x100, if_index=2, sampling=1, direction=1, dscp=64, tls_types=2)
    parts = {"dns": dns(10_000_000, 1, 0x8001, 3, b"\x03www\x03com"), "drops": drops(100, 10, 5, 0x200, 6),
             "xlat": xlat(V4MAP + bytes([1, 2, 3, 4]), V4MAP + bytes([5, 6, 7, 8]), 1, 2, 100),
             "additional": additional(10_000_000, 0, 1), "quic": quic(1, 1, 0)}
    records = np.frombuffer(rec, dtype=np.uint8)
    soa = {k: np.frombuffer(v, dtype=np.uint8) for k, v in parts.items()}
    buf, off, deferred = R.encode(records, np.array([0xFF], dtype=np.uint8), soa, NOW, MONO, NAMES, AGENT, RECEIVED)
    assert off.tolist() == [0, len(buf)] and deferred.tolist() == [0]
    assert buf == (
        b'{"AgentIP":"10.9.8.7","Bytes":456,"DnsErrno":3,"DnsFlags":32769,"DnsFlagsResponseCode":"FormErr","DnsId":1,"DnsLatencyMs":10,'
        b'"DnsName":"www.com","Dscp":64,"DstAddr":"10.11.12.13","DstMac":"00:00:00:00:00:00","DstPort":443,"Etype":2048,"Flags":256,'
        b'"IPSecRetCode":0,"IPSecStatus":"success","IfDirections":[1],"Interfaces":["eth0"],"Packets":123,"PktDropBytes":100,'
        b'"PktDropLatestDropCause":"SKB_DROP_REASON_TCP_CSUM","PktDropLatestFlags":512,"PktDropLatestState":"TCP_CLOSE","PktDropPackets":10,'
        b'"Proto":6,"QuicSeenLongHdr":1,"QuicSeenShortHdr":0,"QuicVersion":"QUIC v2","Sampling":1,"SrcAddr":"6.7.8.9",'
        b'"SrcMac":"00:00:00:00:00:00","SrcPort":23000,"TLSTypes":["ServerHello"],"TimeFlowEndMs":1700000000123,"TimeFlowRttNs":10000000,'
        b'"TimeFlowStartMs":1700000000123,"TimeReceived":1700000000,"Udns":[""],"XlatDstAddr":"5.6.7.8","XlatDstPort":2,'
        b'"XlatSrcAddr":"1.2.3.4","XlatSrcPort":1,"ZoneId":100}\n')
    # present bits and missing arrays both take a part away; network events never add anything
    none = R.encode(records, np.array([8], dtype=np.uint8), soa, NOW, MONO, NAMES, AGENT, RECEIVED)[0]
    assert none == R.encode(records, None, None, NOW, MONO, NAMES, AGENT, RECEIVED)[0]
    assert none == R.encode(records, np.array([0xFF], dtype=np.uint8), {}, NOW, MONO, NAMES, AGENT, RECEIVED)[0]
    assert b"Dns" not in none and b"Quic" not in none and none.endswith(b',"Udns":[""]}\n')


def test_name_tables_sizes_and_ends():
    assert len(R.RCODES) == 11 and len(R.TCP_STATES) == 11 and len(R.CORE_CAUSES) == 79 and len(R.OVS_CAUSES) == 11
    assert len(R.NETWORK_EVENT_CAUSES) == 10
    assert R.drop_cause(4) == b"SKB_DROP_REASON_PKT_TOO_SMALL" and R.drop_cause(48) == b"SKB_DROP_REASON_XDP"
    assert R.drop_cause(66) == b"SKB_DROP_REASON_DUP_FRAG" and R.drop_cause(76) == b"SKB_DROP_REASON_QUEUE_PURGE"
    longest = max(len(R.drop_cause(c)) for c in list(range(0, 100)) + [(3 << 16) + k for k in range(13)] + [(1 << 24) + k for k in range(11)])
    assert longest == 39                                   # what the encoder's longest-line bound takes for the cause


# ---- the C ABI: exported, declared, and refusing bad arguments before any device work

def test_entry_points_are_exported_and_declared(nf):
    L = nf._lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nfagg.h")).read()
    for name in ("nfagg_encode_flp_json_content", "nfagg_encode_flp_json_content_device"):
        assert name + "(" in header and name in L.SIGNATURES and getattr(L.lib, name)
    assert L.lib.nfagg_abi_version() == 2
    assert callable(nf.FlowTable.encode_flp_json_content) and callable(nf.FlowTable.encode_flp_json_content_device)


@pytest.mark.parametrize("device", [False, True])
def test_content_encode_rejects_bad_arguments_before_device_work(nf, device):
    L = nf._lib
    fn = L.lib.nfagg_encode_flp_json_content_device if device else L.lib.nfagg_encode_flp_json_content
    off = np.zeros(2, dtype=np.uint64)
    need, n_def = C.c_size_t(0), C.c_size_t(0)
    rec = np.zeros(1, dtype=nf.FLOW_RECORD)
    feat = L.PbFeatures()
    feat.struct_size = C.sizeof(L.PbFeatures)

    def call(o, f=feat):
        return fn(None, rec.ctypes.data_as(C.c_void_p), 1, C.byref(f) if f is not None else None, C.byref(o) if o is not None else None,
                  None, 0, off.ctypes.data_as(C.c_void_p), None, C.byref(n_def), C.byref(need))

    assert call(None) == L.EINVAL and b"null options" in L.lib.nfagg_last_error(None)
    o, keep = nf.flp_options(names=nf.intf_table([(1, None, "lo", "")]))
    o.struct_size += 8
    assert call(o) == L.EINVAL and b"nfagg_flp_options.struct_size" in L.lib.nfagg_last_error(None)
    bad = nf.intf_table([(1, None, "lo", "x")])
    bad[0]["udn_len"] = 64
    o, keep = nf.flp_options(names=bad)
    assert call(o) == L.EINVAL and b"row 0: udn too long" in L.lib.nfagg_last_error(None)
    o, keep = nf.flp_options(agent_ip=AGENT)
    for f in (feat, None):                                # good options, no handle; features == NULL is allowed
        assert call(o, f) == L.EINVAL and b"null argument" in L.lib.nfagg_last_error(None)
    assert not off.any() and need.value == 0
