"""extract conntrack's lines on the device, CPU side. Flow logs (nfagg_encode_flp_json_conn): the symbols and their signatures, the
longest line of the three policies and the window it leaves, the argument checks that end a call before any device work, the new
kernels' LDS in the shipped code objects, a self-check of the splice helper. Conversation records (nfagg_encode_conn_json): the
restatement of tests/conn_json_ref.py against the hand-written lines of tests/golden/conn_lines_vectors.json, the layout with no
handle (sort order around the blocks, every refusal, the caps, a key-named field, the line cap), the struct sizes, ConnTrack.layout."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = b',"_HashId":"%s","_RecordType":"flowLog"'


def test_symbols_and_signatures(nf):
    L = nf._lib
    assert L.lib.nfagg_abi_version() == 2
    for sym in ("nfagg_encode_flp_json_conn", "nfagg_encode_flp_json_conn_device", "nfagg_flp_json_conn_max_line"):
        assert getattr(L.lib, sym) is not None and sym in L.SIGNATURES
    net, conn = L.SIGNATURES["nfagg_encode_flp_json_net"][1], L.SIGNATURES["nfagg_encode_flp_json_conn"][1]
    assert len(conn) == len(net) + 1 and conn[:9] == net[:9] and conn[10:] == net[9:]          # the ids behind the net table
    assert L.SIGNATURES["nfagg_encode_flp_json_conn_device"] == L.SIGNATURES["nfagg_encode_flp_json_conn"]
    for name in ("encode_flp_json_conn", "encode_flp_json_conn_device"):
        assert callable(getattr(nf.FlowTable, name))


@pytest.mark.parametrize("policy", [0, 1, 2])
def test_longest_line_and_the_window_it_leaves(nf, policy):
    lib = nf._lib.lib
    grow = len(KEYS % (b"f" * 16))
    assert grow == 53 and lib.nfagg_flp_json_conn_max_line(policy) == lib.nfagg_flp_json_net_max_line(policy) + grow
    assert lib.nfagg_flp_json_conn_max_line(3) == 0 and lib.nfagg_flp_json_conn_max_line(-1) == 0
    line = (lib.nfagg_flp_json_conn_max_line(policy) + 15) // 16 * 16
    window = (32768 - (16 if policy == 0 else 2048) - line) // 16 * 16                             # FlpConnMeta<Base>::kWindow
    assert window >= 16384 and window + line + (16 if policy == 0 else 2048) <= 32768


def test_calls_end_at_their_argument_checks_without_a_handle(nf):
    L = nf._lib
    with nf.NetTable(7) as net, nf.TlsNames() as tls, nf.K8sTable([]) as k8s:
        o, keep = nf.flp_options(agent_ip=bytes(16))
        off, need, ids = np.zeros(2, dtype=np.uint64), C.c_size_t(7), np.zeros(1, dtype=np.uint64)
        for fn in (L.lib.nfagg_encode_flp_json_conn, L.lib.nfagg_encode_flp_json_conn_device):
            assert fn(None, None, 0, None, None, None, tls._t, k8s._t, net._t, ids.ctypes.data_as(C.c_void_p), C.byref(o), None, 0,
                      off.ctypes.data_as(C.c_void_p), C.byref(need)) == L.EINVAL
            assert fn(None, None, 0, None, None, None, tls._t, k8s._t, net._t, ids.ctypes.data_as(C.c_void_p), None, None, 0,
                      off.ctypes.data_as(C.c_void_p), C.byref(need)) == L.EINVAL
            assert b"null options" in L.lib.nfagg_last_error(None)
        assert need.value == 7 and not off.any()


def test_the_conn_kernels_are_flp_instantiations_within_32_kib_of_lds_and_no_copied_pair_is_left(tmp_path):
    """One size and one write kernel per policy, as instantiations of k_flp_size / k_flp_write over FlpConnMeta; read from the code
    objects' metadata notes as tests/test_isa_pins.py reads k_flp_write's. The kernel pairs the levels above TLS once had under
    names of their own are gone from the library."""
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = os.path.join(os.path.dirname(objdump), "llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no llvm-objdump / llvm-readelf in this image")
    lib = os.path.join(os.path.dirname(HERE), "netobserv-ebpf-agent_amd", "lib", "libnfagg.so")
    shutil.copy(lib, tmp_path / "libnfagg.so")
    subprocess.check_call([objdump, "--offloading", "libnfagg.so"], cwd=tmp_path, stdout=subprocess.DEVNULL)
    found, names = {}, []
    for co in sorted(glob.glob(str(tmp_path / "libnfagg.so.*gfx950*"))):
        notes = subprocess.check_output([readelf, "--notes", co], text=True)
        for entry in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            field = lambda key: re.search(r"\.%s:\s+(\S+)" % key, entry).group(1)      # noqa: E731
            names.append(field("name"))
            if re.search(r"k_flp_(size|write)I", field("name")) and "FlpConnMeta" in field("name"):
                found[field("name")] = int(field("group_segment_fixed_size"))
    write = {k: v for k, v in found.items() if "k_flp_write" in k}
    assert len(found) == 6 and len(write) == 3, sorted(found)
    assert all("FlpConnMeta" in k and "FlpNet" in k for k in found)
    assert all(16384 < lds <= 32768 for lds in write.values()), write
    assert len(names) > 100, "kernel names not read: %d" % len(names)
    left = [k for k in names if re.search(r"k_k8s_size|k_k8s_write|k_net_size|k_net_write|k_connlog_", k)]
    assert not left, left


def test_the_splice_on_hand_written_lines(nf):
    """A self-check of the tests' own helper (tests/conn_lines_ref.py), not of the product: three lines written by hand, a tracked
    flow with id 0, an untracked flow, a tracked flow with sixteen digits."""
    import conn_lines_ref as CL
    recs = np.zeros(3, dtype=nf.FLOW_RECORD)
    recs["metrics"]["eth_protocol"] = [0x0800, 0x0800, 0x86DD]
    recs["id"]["transport_protocol"] = [6, 1, 132]
    lines = [b'{"A":1}\n', b'{"B":[]}\n', b'{"Udns":[""],"ZoneId":7}\n']
    off = np.cumsum([0] + [len(x) for x in lines]).astype(np.uint64)
    buf, got = CL.splice((b"".join(lines), off), recs, [0, 5, (1 << 64) - 1])
    want = [b'{"A":1,"_HashId":"0","_RecordType":"flowLog"}\n', b"", b'{"Udns":[""],"ZoneId":7,"_HashId":"ffffffffffffffff","_RecordType":"flowLog"}\n']
    assert buf == b"".join(want) and got.tolist() == [0, len(want[0]), len(want[0]), len(want[0]) + len(want[2])]
    assert CL.tracked(recs).tolist() == [True, False, True]


# ---- conversation records: the restatement against hand-written lines, the layout with no handle, the struct sizes
import json  # noqa: E402

import conn_cases as CC  # noqa: E402
import conn_json_ref as CJ  # noqa: E402
import flp_json_net_ref as R  # noqa: E402

VECTORS = json.load(open(os.path.join(HERE, "golden", "conn_lines_vectors.json")))["vectors"]


def spec_of(v):
    kw = dict(v["conv"])
    for which in ("first", "last"):
        if which in kw:
            s = dict(kw[which])
            if "smac" in s:
                s["smac"] = bytes.fromhex(s["smac"])
            kw[which] = CC.snap(**s)
    for k in ("flows", "nbytes", "packets"):
        if k in kw:
            kw[k] = tuple(kw[k])
    return CC.conv(**kw)


@pytest.mark.parametrize("v", VECTORS, ids=[v["name"] for v in VECTORS])
def test_restatement_against_hand_written_lines(v):
    args = (v["fields"], CC.ref_conv(spec_of(v)), {}, None, R.RULES_OFF, [])
    if v["want"] is None:
        with pytest.raises(CJ.Deferred):
            CJ.line(*args)
    else:
        assert CJ.line(*args) == v["want"].encode() + b"\n"


def test_restatement_applies_the_rules_behind_conntrack():
    import flp_json_k8s_ref as K
    table = K.table_of([("10.0.0.1", dict(namespace="shop", name="cart", kind="Pod", host_ip="192.168.1.10"))])
    cats = R.parse_subnets([(b"lan", ["10.0.0.0/24"])])
    line = CJ.line([dict(name="numFlowLogs", operation="count")], CC.ref_conv(CC.conv()), table, None, dict(R.RULES_OFF, direction=True, labels=[("lan", ["10.0.0.0/24"])]), cats)
    assert b'"SrcK8S_Name":"cart"' in line and b'"SrcSubnetLabel":"lan"' in line and b'"DstSubnetLabel":"lan"' in line and b"FlowDirection" not in line
    assert CJ.marshal({b"b": True, b"a": 3.0, b"c": [1, 2], b"_": False}) == b'{"_":false,"a":3,"b":true,"c":[1,2]}'
    for bad in (float(1 << 53), -float(1 << 53), 0.5):
        with pytest.raises(CJ.Deferred):
            CJ.marshal({b"x": bad})


def test_layout_sort_order_around_the_blocks(nf):
    names = ["DstB", "DstK8", "DstK9", "DstMac", "_Foo", "a", "SrcK8", "SrcL", "K8S_FlowLaye", "K8S_FlowLayes", "DstSubnetLabe", "DstSubnetLabel2", "_I", "_Z"]
    with nf.ConnLayout([dict(name=n, operation="count") for n in names]) as lay:
        got = [lay.render(k) for k in range(lay.n_columns)]
    blocks = {"DstK8S_": 0, "DstSubnetLabel": 1, "K8S_FlowLayer": 2, "SrcK8S_": 3, "SrcSubnetLabel": 4}
    every = sorted(names + ["SrcAddr", "DstAddr", "SrcPort", "DstPort", "Proto", "_HashId", "_IsFirst", "_RecordType"] + list(blocks), key=lambda s: s.encode())
    assert got == [b"" if n in blocks else b',"%s":' % n.encode() for n in every] and lay.n_columns == len(names) + 13
    assert every.index("DstK8") < every.index("DstK8S_") < every.index("DstK9") and every.index("_Foo") < every.index("_HashId") < every.index("_I")
    with nf.ConnLayout([dict(name=b'q"\x01\xff', operation="count")]) as lay:
        assert b',"q\\"\\u0001\xff":' in [lay.render(k) for k in range(lay.n_columns)]


@pytest.mark.parametrize("fields, text", [
    ([dict(name="SrcK8S_x", operation="count")], "SrcK8S_x"), ([dict(name="DstK8S_", operation="count")], "DstK8S_"),
    ([dict(name="K8S_FlowLayer", operation="count")], "K8S_FlowLayer"), ([dict(name="SrcSubnetLabel", operation="count")], "SrcSubnetLabel"),
    ([dict(name="DstSubnetLabel", operation="count")], "DstSubnetLabel"), ([dict(name="_HashId", operation="count")], "_HashId"),
    ([dict(name="_IsFirst", operation="count")], "_IsFirst"), ([dict(name="_RecordType", operation="count")], "_RecordType"),
    ([dict(name="", operation="count")], "empty name"), ([dict(name="x" * 65, operation="count")], "65 bytes"),
    ([dict(name="a", operation="count"), dict(name="a", operation="sum", input="Bytes")], "duplicate name a"),
    ([dict(name="a_AB", operation="count"), dict(name="a", operation="count", splitAB=True)], "duplicate name a_AB"),
    ([dict(name="s", operation="sum", input="Proto")], "(s)"), ([dict(name="s", operation="sum")], "(s)"),
    ([dict(name="m", operation="min", input="Bytes")], "(m)"), ([dict(name="m", operation="min", input="TimeFlowStartMs", splitAB=True)], "(m)"),
    ([dict(name="m", operation="max", input="TimeFlowStartMs")], "(m)"), ([dict(name="f", operation="first", input="Bytes")], "(f)"),
    ([dict(name="f", operation="first", input="Interfaces")], "(f)"), ([dict(name="f", operation="last", input="SrcMac", splitAB=True)], "(f)"),
    ([dict(name="o", operation="median")], "(o)"), ([dict(name="f%d" % k, operation="count") for k in range(33)], "33 output fields")])
def test_layout_refuses(nf, fields, text):
    with pytest.raises(nf.NfaggError) as e:
        nf.ConnLayout(fields)
    assert e.value.code == nf._lib.EINVAL and text in str(e.value)


def test_layout_caps_a_key_named_field_and_the_line_cap(nf):
    with nf.ConnLayout([dict(name="f%d" % k, operation="count") for k in range(32)]) as lay:
        assert lay.n_columns == 32 + 13
    with nf.ConnLayout([dict(name="x" * 64, operation="count", splitAB=True)]) as lay:
        assert lay.render(lay.n_columns - 1) == b',"' + b"x" * 64 + b'_BA":'
    with nf.ConnLayout([dict(name="SrcPort", operation="first", input="DstPort"), dict(name="Proto", operation="count")]) as lay, nf.ConnLayout([]) as none:
        assert lay.n_columns == none.n_columns == 13 and lay.max_line == none.max_line                # the keys prevail
    with nf.ConnLayout(CC.FIELDS_32) as lay:
        assert lay.max_line <= 32768 - 16 - 16384
    with pytest.raises(nf.NfaggError) as e:                        # 64 columns whose names escape to 6 bytes a byte
        nf.ConnLayout([dict(name=b"\x01" * 63 + bytes([65 + k]), operation="sum", input="Bytes", splitAB=True) for k in range(32)])
    assert e.value.code == nf._lib.ERANGE and "more than 16368" in str(e.value)


def test_conversation_struct_sizes(nf, tmp_path):
    L = nf._lib
    assert (nf.CONN_VALUES.itemsize, nf.CONN_SNAPSHOT.itemsize, C.sizeof(L.ConnField)) == (256, 80, 16)
    assert (nf.CONN_VALUES.fields["first"][1], nf.CONN_VALUES.fields["last"][1], nf.CONN_SNAPSHOT.fields["start_ms"][1]) == (80, 160, 64)
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nfagg.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(nfagg_conn_values), '
                   'sizeof(nfagg_conn_snapshot), sizeof(nfagg_conn_field), offsetof(nfagg_conn_values, first), offsetof(nfagg_conn_values, last), '
                   'offsetof(nfagg_conn_snapshot, n_dirs));return 0;}\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(tmp_path / "p")])
    assert subprocess.check_output([str(tmp_path / "p")], text=True).split() == ["256", "80", "16", "80", "160", "52"]
    for sym in ("nfagg_conn_layout_create", "nfagg_conn_layout_destroy", "nfagg_conn_layout_render", "nfagg_encode_conn_json", "nfagg_encode_conn_json_device"):
        assert getattr(L.lib, sym) is not None and sym in L.SIGNATURES


def test_conntrack_layout_takes_what_the_mirror_serves(nf):
    """ConnTrack.layout: every field conntrack._served accepts compiles, a split field gives two columns, and a field the
    mirror refuses never reaches the layout."""
    import test_conntrack_cpu as T
    fields = [dict(name="Bytes", operation="sum", splitAB=True), dict(name="Packets", operation="sum"), dict(name="numFlowLogs", operation="count", splitAB=True),
              dict(name="TimeFlowStartMs", operation="min"), dict(name="TimeFlowEndMs", operation="max")]
    fields += [dict(name="first_" + i, operation="first", input=i) for i in nf.conntrack.FIRST_LAST_FIELDS]
    fields += [dict(name="last_" + i, operation="last", input=i) for i in nf.conntrack.FIRST_LAST_FIELDS]
    cfg = dict(T.config(), outputFields=fields)
    with nf.ConnTrack(cfg).layout() as lay:
        assert lay.n_columns == 13 + len(fields) + 2 and lay.render(0) == b',"Bytes_AB":'
    with pytest.raises(ValueError):
        nf.ConnTrack(dict(cfg, outputFields=[dict(name="x", operation="first", input="Interfaces")]))
