"""Network events without a GPU: the restatement of record.go:126-157 (tests/netev_ref.py) against the reference's two known
answers (tests/golden/netev_vectors.json), and the host side of the cookie table (nfagg_netev_render,
nfagg_netev_table_create with a NULL handle): rendered bytes against the restatement and against the Python protobuf
runtime, every escape class of jsoniter's WriteString, the 512-byte cap on both sides, the duplicate-cookie error."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import netev_ref as N  # noqa: E402

VEC = json.load(open(os.path.join(HERE, "golden", "netev_vectors.json")))


def acl(d):
    return (d["action"], d["actor"], d["name"], d["namespace"], d["direction"], d["string"])


def fake_decoder(cookie: bytes):
    return acl(VEC["decoder"]["cookie0_is_1" if cookie[0] == 1 else "otherwise"])


def kat_inputs(O, case):
    ne = np.zeros(1, dtype=O.NETEV)
    for k, c in enumerate(case["network_events"]["cookies"]):
        ne["network_events"][0, k] = np.frombuffer(bytes.fromhex(c), dtype=np.uint8)
    ne["bytes"][0], ne["packets"][0] = case["network_events"]["bytes"], case["network_events"]["packets"]
    ne["network_events_idx"] = case["network_events"]["network_events_idx"]
    present = np.array([N.FEAT_NETEV], dtype=np.uint8)
    drops = None
    if case["drops"] is not None:
        drops = np.zeros(1, dtype=O.DROPS)
        for k, v in case["drops"].items():
            drops[k] = v
        present |= N.FEAT_DROPS
    return present, ne, drops


@pytest.mark.parametrize("case", VEC["cases"], ids=[c["name"] for c in VEC["cases"]])
def test_restatement_matches_the_reference_kats(O, case):
    present, ne, drops = kat_inputs(O, case)
    (p_out, d_out, rows, events, missing), answers, calls = N.resolve_loop(present, ne, drops, fake_decoder)
    assert calls == 2 and not missing
    want = [{k.encode(): v.encode() for k, v in m.items()} for m in case["expect_events"]]
    assert [N.to_map(e) for e in events[0]] == want
    d = d_out.view(O.DROPS).reshape(-1)[0]
    assert p_out[0] & N.FEAT_DROPS
    for k, v in case["expect_drops"].items():
        assert int(d[k]) == v, k
    assert int(d["start"]) == 0 and int(d["end"]) == 0 and int(d["eth_protocol"]) == 0
    assert N.CAUSES[int(d["latest_drop_cause"]) - (1 << 24)] == case["expect_cause_name"]
    order = N.table_rows(answers)
    assert rows[0].tolist() == [order[bytes.fromhex(c)] for c in case["network_events"]["cookies"][:2]] + [N.NO_ROW] * 2


# ---- the rendered bytes
EVENTS = {
    "reference-acl": acl(VEC["decoder"]["otherwise"]),
    "empty-strings": ("", "", "", "", "", ""),
    "message": b"Custom event from an OVN sample",
    "empty-message": b"",
    "escapes": (b'dr"op', b"back\\slash", b"new\nline\r\ttab", b"\x01\x1f below 0x20", b"\x7f\x80\xc3\xa9\xff up", b"s"),
    "message-escapes": b'q" \\ \n \x00 \xff',
    "two-63-byte-names": ("allow-related", "AdminNetworkPolicy", "n" * 63, "s" * 63, "Egress", "x"),
}


def _netevent_class():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    T = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto()
    fd.name, fd.package, fd.syntax = "netev_flow.proto", "pbflow", "proto3"
    m = fd.message_type.add(); m.name = "NetworkEvent"
    e = m.nested_type.add(); e.name = "EventsEntry"; e.options.map_entry = True
    for name, num in (("key", 1), ("value", 2)):
        f = e.field.add(); f.name, f.number, f.type, f.label = name, num, T.TYPE_STRING, T.LABEL_OPTIONAL
    f = m.field.add(); f.name, f.number, f.type, f.label, f.type_name = "events", 1, T.TYPE_MESSAGE, T.LABEL_REPEATED, ".pbflow.NetworkEvent.EventsEntry"
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("pbflow.NetworkEvent"))


@pytest.mark.parametrize("name", sorted(EVENTS))
def test_render_matches_the_restatement(nf, name):
    ev = EVENTS[name]
    assert nf.netev_render(ev, nf._lib.NETEV_JSON) == N.render_json(ev)
    assert nf.netev_render(ev, nf._lib.NETEV_PB) == N.render_pb(ev)


def test_reference_object_reads_back(nf):
    got = nf.netev_render(EVENTS["reference-acl"], nf._lib.NETEV_JSON)
    assert len(got) == 115
    assert json.loads(got) == VEC["cases"][0]["expect_events"][1]
    assert list(json.loads(got)) == sorted(json.loads(got))


def _entries(buf: bytes):
    """The top-level map entries of a serialized NetworkEvent, each with its tag and length."""
    out, i = [], 0
    while i < len(buf):
        assert buf[i] == 0x0A
        ln, j = N._read_varint(buf, i + 1)
        out.append(buf[i:j + ln])
        i = j + ln
    return out


@pytest.mark.parametrize("name", ["reference-acl", "empty-strings", "message", "empty-message", "two-63-byte-names"])
def test_render_pb_matches_the_protobuf_runtime(nf, name):
    """Second opinion on the serialized pbflow.NetworkEvent: google.protobuf with deterministic=True. Valid UTF-8 events only:
    the runtime refuses anything else in a string field. Every map entry must be the runtime's entry byte for byte, and the
    runtime must read the rendering back as the same map. The ORDER of the entries is compared only where no key is a prefix
    of another: this runtime (upb 7.35.1) puts the longer of two such keys first ("Namespace" before "Name"), Go's
    deterministic marshal orders map keys with the plain string comparison (internal/order, GenericKeyOrder), shorter
    first, and that is the order the library renders."""
    ev = EVENTS[name]
    msg = _netevent_class()()
    for k, v in N.to_map(ev).items():
        msg.events[k.decode()] = v.decode()
    want = msg.SerializeToString(deterministic=True)
    got = nf.netev_render(ev, nf._lib.NETEV_PB)
    assert sorted(_entries(got)) == sorted(_entries(want))
    keys = sorted(N.to_map(ev))
    heads = [e[N._read_varint(e, 1)[1]:] for e in _entries(got)]                  # 0x0A klen key ...: keys in byte order
    assert [h[2:2 + h[1]] for h in heads] == keys
    if not any(a != b and b.startswith(a) for a in keys for b in keys):
        assert got == want
    back = _netevent_class()()
    back.ParseFromString(got)
    assert dict(back.events) == {k.decode(): v.decode() for k, v in N.to_map(ev).items()}


def test_render_refuses_an_undecodable_entry(nf):
    with pytest.raises(nf.NfaggError) as e:
        nf.netev_render(None, nf._lib.NETEV_JSON)
    assert e.value.code == nf._lib.EINVAL


# ---- the cap: {"Message":"..."} is 14 bytes around the escaped string; the message 0x0A len {0x0A 7 "Message" 0x12 len v} is
# 3 + 9 + 3 + len(v) bytes once both lengths take two bytes
@pytest.mark.parametrize("fmt, at_cap", [("NETEV_JSON", 512 - 14), ("NETEV_PB", 512 - 15)])
def test_cap_on_both_sides(nf, fmt, at_cap):
    f = getattr(nf._lib, fmt)
    ok = b"m" * at_cap
    assert len(nf.netev_render(ok, f)) == 512
    assert len(N.render_json(ok) if fmt == "NETEV_JSON" else N.render_pb(ok)) == 512
    with pytest.raises(nf.NfaggError) as e:
        nf.netev_render(ok + b"m", f)
    assert e.value.code == nf._lib.EINVAL and "512" in str(e.value)


def test_cap_counts_escaped_bytes(nf):
    """249 quotes escape to 498 bytes: the object is at the cap although the message has 249 bytes; the protobuf message copies
    them as they are."""
    ok = b'"' * 249
    assert len(nf.netev_render(ok, nf._lib.NETEV_JSON)) == 512
    with pytest.raises(nf.NfaggError):
        nf.netev_render(ok + b"a", nf._lib.NETEV_JSON)
    assert len(nf.netev_render(ok + b"a", nf._lib.NETEV_PB)) == 3 + 9 + 3 + 250


def test_table_build_names_the_row_over_the_cap(nf):
    good = (bytes([1] + [0] * 7), EVENTS["reference-acl"])
    with nf.NetevTable([good, (bytes([2] + [0] * 7), b"m" * 497)]) as t:
        assert len(t) == 2
    with pytest.raises(nf.NfaggError) as e:
        nf.NetevTable([good, (bytes([2] + [0] * 7), None), (bytes([3] + [0] * 7), b"m" * 499)])
    assert e.value.code == nf._lib.EINVAL and "entry 2" in str(e.value) and "512" in str(e.value)
    big_acl = ("allow", "NetworkPolicy", "n" * 300, "s" * 300, "Ingress", "x")
    with pytest.raises(nf.NfaggError) as e:
        nf.NetevTable([(bytes(8), big_acl)])
    assert "entry 0" in str(e.value)


def test_duplicate_cookies_are_an_error(nf):
    c = bytes.fromhex("0102030405060708")
    with pytest.raises(nf.NfaggError) as e:
        nf.NetevTable([(c, b"one"), (bytes(8), b"zero"), (c, b"two")])
    assert e.value.code == nf._lib.EINVAL and "same cookie" in str(e.value) and "0 and 2" in str(e.value)
    with nf.NetevTable([(c, b"one"), (bytes(8), b"zero"), (c[::-1], None)]) as t:
        assert t.cookies == sorted([c, bytes(8), c[::-1]], key=N.cookie_value)
    with nf.NetevTable([]) as t:
        assert len(t) == 0
