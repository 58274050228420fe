"""write ipfix on the device, the parts that need no GPU: the template messages against prepareTemplate's element lists, the
flag identity the flags_decoded option rests on, the strings table's host build and its refusals, the bindings, the restatement's
own carry (tests/flp_ipfix_ref.py is what the GPU tests compare with), and the C driver of the host-only entry points."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_ipfix_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("enterprise", [0, 2, 0x7FFFFFFF])
@pytest.mark.parametrize("v6", [False, True])
def test_template_decodes_to_prepare_template(nf, v6, enterprise):
    msg = nf.flp_ipfix_template(v6, 1_700_000_000, 7, enterprise)
    rec, elements = R.prepare_template(257 if v6 else 256, enterprise, v6)
    assert msg == R.message(2, rec, 1, 7, 1_700_000_000)
    tid, fields = R.parse_template(msg)
    assert tid == (257 if v6 else 256)
    assert fields == [(e.id, e.len, e.enterprise) for e in elements]
    assert len(fields) == (24 if v6 else 23) + (9 if enterprise else 0)
    names = [e.name for e in elements]
    assert names[:2] == (["sourceIPv6Address", "destinationIPv6Address"] if v6 else ["sourceIPv4Address", "destinationIPv4Address"])
    if enterprise:
        assert names[-9:] == ["sourcePodNamespace", "sourcePodName", "destinationPodNamespace", "destinationPodName", "sourceNodeName",
                              "destinationNodeName", "timeFlowRttNs", "interfaces", "directions"]
        assert [f[1] for f in fields[-9:]] == [65535] * 6 + [8, 65535, 65535]


def test_template_ids_and_domain_are_the_options(nf):
    msg = nf.flp_ipfix_template(True, 5, 0xFFFFFFFF, 9, obs_domain_id=77, template_ids=(300, 301))
    assert struct.unpack_from(">HHIII", msg, 0) == (10, len(msg), 5, 0xFFFFFFFF, 77)
    assert R.parse_template(msg)[0] == 301


def test_encode_of_decode_is_the_low_eleven_bits():
    for x in range(1 << 16):
        assert R.encode_tcp_flags(R.decode_tcp_flags(x)) == x & 0x7FF
    assert R.decode_tcp_flags(0x800) == [] and R.encode_tcp_flags([b"nope"]) == 0


def _entries(**fields):
    info = dict(namespace="ns", name="pod", host_ip="10.0.0.1", host_name="node")
    info.update(fields)
    return [("10.1.0.1", info)]


def test_strings_table_host_build_and_refusals(nf):
    for field in ("namespace", "name", "host_name"):
        for ln in (0, 1, 254, 255, 256, 1024):
            with nf.IpfixStrings(_entries(**{field: (bytes(range(256)) * 4)[:ln]})) as t:
                assert len(t) == 1
        with pytest.raises(nf.NfaggError) as e:
            nf.IpfixStrings(_entries(**{field: b"y" * 1025}))
        assert e.value.code == nf._lib.EINVAL and "1025 bytes, more than 1024" in str(e.value)
    with nf.IpfixStrings([]) as t:
        assert len(t) == 0
    L = nf._lib
    e = L.K8sEntry()
    e.name, e.name_len = None, 3                                   # a null pointer with a length
    out = C.c_void_p()
    assert L.lib.nfagg_flp_ipfix_strings_create(None, C.byref(e), 1, C.byref(out)) == L.EINVAL and not out.value
    assert b"name is null with a length" in L.lib.nfagg_last_error(None)
    assert L.lib.nfagg_flp_ipfix_strings_create(None, None, 1, C.byref(out)) == L.EINVAL


def test_symbols_signatures_and_sizes(nf):
    L = nf._lib
    for sym in ("nfagg_flp_ipfix_template", "nfagg_flp_ipfix_strings_create", "nfagg_flp_ipfix_strings_destroy", "nfagg_flp_ipfix_writer_create",
                "nfagg_flp_ipfix_writer_destroy", "nfagg_flp_ipfix_writer_get", "nfagg_flp_ipfix_writer_reset", "nfagg_flp_ipfix_write",
                "nfagg_flp_ipfix_write_device"):
        assert sym in L.SIGNATURES and getattr(L.lib, sym)
    assert L.SIGNATURES["nfagg_flp_ipfix_write"] == L.SIGNATURES["nfagg_flp_ipfix_write_device"]
    assert C.sizeof(L.FlpIpfixElements) == 9424 and L.FlpIpfixElements.str.offset == 208
    header = open(os.path.join(ROOT, "include", "nfagg.h")).read()
    assert "#define NFAGG_FLP_IPFIX_MAX_STRING %d" % L.FLP_IPFIX_MAX_STRING in header
    assert hasattr(nf.FlowTable, "flp_ipfix_write") and hasattr(nf.FlowTable, "flp_ipfix_writer") and hasattr(nf.FlowTable, "flp_ipfix_strings")


def test_struct_layouts_match_the_header(nf, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nfagg.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(nfagg_flp_ipfix_options), offsetof(nfagg_flp_ipfix_options, export_time_s), offsetof(nfagg_flp_ipfix_options, max_msg_size), '
                   'sizeof(nfagg_flp_ipfix_elements), offsetof(nfagg_flp_ipfix_elements, sampling_probability)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    L = nf._lib
    assert got == [C.sizeof(L.FlpIpfixOptions), L.FlpIpfixOptions.export_time_s.offset, L.FlpIpfixOptions.max_msg_size.offset,
                   C.sizeof(L.FlpIpfixElements), L.FlpIpfixElements.sampling_probability.offset]


def test_write_ipfix_config_defaults_and_checks(nf):
    W = nf.WriteIpfix
    for bad in ({}, dict(targetHost="h"), dict(targetHost="h", targetPort=1, transport="sctp")):
        with pytest.raises(ValueError):
            W(None, bad, lambda m: None)


def _flow(etype=0x0800, **keys):
    m = {b"Etype": etype, b"SrcMac": b"02:00:00:00:00:01", b"DstMac": b"02:00:00:00:00:02", b"TimeFlowStartMs": 1, b"TimeFlowEndMs": 2,
         b"IfDirections": [1], b"Interfaces": [b"eth0"]}
    m.update({k.encode(): v for k, v in keys.items()})
    return m


def test_restatement_carries_fails_and_counts():
    """The restatement's own behaviour on hand-made maps: what the device is compared with."""
    sent = []
    w = R.WriteIpfix(sent.append, enterprise_id=2, max_msg_size=512, export_time=9)
    assert len(sent) == 2 and R.parse_template(sent[0])[0] == 256 and R.parse_template(sent[1])[0] == 257
    templates = dict(R.parse_template(m) for m in sent)
    assert w.write(_flow(0x0806), 9) is None and w.failures == [(0, 1)] and w.seq == 0       # nil addresses: no To4()
    m1 = w.write(_flow(SrcAddr=b"10.0.0.1", DstAddr=b"10.0.0.2", Proto=6, SrcPort=80, DstPort=81, Flags=0x812, Bytes=5, Sampling=3), 9)
    hdr, vals = R.decode_data(m1, templates)
    assert hdr["seq"] == 0 and hdr["template"] == 256 and w.seq == 1
    by_id = {(eid, ent): v for eid, ent, v in vals}
    assert by_id[(8, 0)] == bytes([10, 0, 0, 1]) and by_id[(1, 0)] == struct.pack(">Q", 5) and by_id[(311, 0)] == struct.pack(">d", 1.0 / 3.0)
    assert by_id[(6, 0)] == struct.pack(">H", 0x812) and by_id[(304, 0)] == struct.pack(">H", 4) and by_id[(225, 0)] == bytes(4)
    m2 = w.write(_flow(0x0806), 9)                                                           # non-IP: every carried value stays
    hdr2, vals2 = R.decode_data(m2, templates)
    assert hdr2["seq"] == 1 and [v for v in vals2 if v[0] != 256] == [v for v in vals if v[0] != 256]       # all but ethernetType
    assert w.write(_flow(SrcAddr=b"2001:db8::1", DstAddr=b"10.0.0.2", Proto=17), 9) is None and w.failures[-1] == (3, 1)
    assert w.elements(False)["sourceIPv4Address"] == R.parse_ip(b"2001:db8::1") and w.seq == 2       # the setters ran
    m6 = w.write(_flow(0x86DD, SrcAddr=b"2001:db8::1", DstAddr=b"::1", Proto=58, IcmpType=128, IcmpCode=0, XlatSrcAddr=b"10.9.9.9",
                       XlatDstAddr=b"2001:db8::2", SrcK8S_Name=b"p" * 255), 9)
    hdr6, vals6 = R.decode_data(m6, templates)
    assert hdr6["template"] == 257 and {(eid, ent): v for eid, ent, v in vals6}[(7734, 2)] == b"p" * 255
    assert m6[m6.index(b"\xff\x00\xffppp"):][:3] == b"\xff\x00\xff"                          # the three-byte length form
    assert w.write(_flow(0x86DD, SrcAddr=b"::2", DstAddr=b"::1", Proto=58, SrcK8S_Name=b"q" * 400), 9) is None and w.failures[-1] == (5, 2)
    assert w.elements(True)["sourcePodName"] == b"q" * 400 and w.seq == 3
    assert R.decode_tcp_flags(0x812) == [b"SYN", b"ACK"]
    w2 = R.WriteIpfix(lambda m: None)
    w2.write(_flow(SrcAddr=b"10.0.0.1", DstAddr=b"10.0.0.2", Proto=6, Flags=R.decode_tcp_flags(0xF812)), 0)
    assert w2.elements(False)["tcpControlBits"] == 0x12


def test_flp_ipfix_host_check_compiles_and_runs(nf, tmp_path):
    lib_dir = os.path.dirname(nf._lib.LIB_PATH)
    exe = str(tmp_path / "flp_ipfix_host_check")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "c", "flp_ipfix_host_check.c"), "-o", exe, "-L", lib_dir, "-lnfagg", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "flp ipfix host check ok", out.stderr
