"""The host side of extract conntrack's lines (conntrack.ConnTrack.conversations, the pieces of format_deferred), without a GPU:
the conversation arrays of a call against the records of tests/conntrack_ref.py's Extract, the float64 digits against hand-written
values and tests/conn_json_ref.float_f, the splitter of a line's members."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conn_json_ref as CJ  # noqa: E402
import conntrack_ref as CT  # noqa: E402
import test_conntrack_cpu as T  # noqa: E402
from flp_json_ref import go_ip, go_mac  # noqa: E402

# strconv.FormatFloat(v, 'f', -1, 64), written by hand: 2^53 is exact, above it the shortest digits and zeros
FLOATS = [(1 << 53, b"9007199254740992"), ((1 << 53) + 2, b"9007199254740994"), (1 << 60, b"1152921504606847000"), (1 << 63, b"9223372036854776000"),
          ((1 << 64) - 1, b"18446744073709552000"), (-(1 << 55), b"-36028797018963970"), (10**20, b"100000000000000000000"), (7, b"7")]


@pytest.mark.parametrize("v, text", FLOATS, ids=[t.decode() for _, t in FLOATS])
def test_float_digits_by_hand(nf, v, text):
    assert nf.conntrack._float_f(v) == text == CJ.float_f(float(v))


def test_float_digits_against_the_restatement(nf):
    rng = np.random.default_rng(5)
    vals = [int(x) >> int(s) for x, s in zip(rng.integers(0, 1 << 64, 4000, dtype=np.uint64), rng.integers(0, 12, 4000))]
    vals += [-v for v in vals[:500]] + [(1 << k) + d for k in range(53, 64) for d in (-1, 0, 1, 3)] + [2 * ((1 << 64) - 1)]
    for v in vals:
        assert nf.conntrack._float_f(v) == CJ.float_f(float(v)), v


def test_members_of_a_line(nf):
    """Commas and quotes inside strings, escaped backslashes at a string's end, an array, an empty string."""
    members = [rb'"a":1', rb'"b,\"x":"q,\\"', rb'"c":[1,2,3]', rb'"d\\":""', rb'"e":true', rb'"f":"\\\",\"g"', rb'"h":-5']
    assert nf.conntrack._members(b"{" + b",".join(members)) == members
    assert nf.conntrack._members(b'{"only":"x"') == [b'"only":"x"']


def conv_of(fields, car, val, types):
    """One conversation of the arrays as the record tests/conntrack_ref.py's Extract returns, decoded here."""
    def values(w):
        return {b"SrcAddr": go_ip(w["src_ip"].tobytes()), b"DstAddr": go_ip(w["dst_ip"].tobytes()), b"SrcPort": int(w["src_port"]), b"DstPort": int(w["dst_port"]),
                b"Proto": int(w["proto"]), b"SrcMac": go_mac(w["src_mac"].tobytes()), b"DstMac": go_mac(w["dst_mac"].tobytes()), b"Etype": int(w["eth_protocol"]),
                b"Dscp": int(w["dscp"]), b"TimeFlowStartMs": int(w["start_ms"]), b"TimeFlowEndMs": int(w["end_ms"]),
                b"IfDirections": [int(x) for x in w["dirs"][:int(w["n_dirs"])]]}
    k = car["id"]
    assert int(car["metrics"]["eth_protocol"]) in (0x0800, 0x86DD)
    m = {}
    for f in fields:
        op, name, inp = f["operation"], f["name"].encode(), (f.get("input", "") or f["name"]).encode()
        if op in ("first", "last"):
            m[name] = values(val[op])[inp]
            continue
        if op in ("min", "max"):
            pairs = [(name, int(val["start_ms_min" if op == "min" else "end_ms_max"]))]
        else:
            ab, ba = (int(x) for x in val["flows" if op == "count" else inp.decode().lower()])
            pairs = [(name + b"_AB", ab), (name + b"_BA", ba)] if f.get("splitAB", False) else [(name, ab + ba)]
        m.update({n: float(v) for n, v in pairs if v != 0})
    m.update({b"SrcAddr": go_ip(k["src_ip"].tobytes()), b"DstAddr": go_ip(k["dst_ip"].tobytes()), b"SrcPort": int(k["src_port"]), b"DstPort": int(k["dst_port"]),
              b"Proto": int(k["transport_protocol"])})
    m.update({b"_HashId": b"%x" % int(val["hash_total"]), b"_RecordType": types[int(val["record_type"])].encode(), b"_IsFirst": bool(val["is_first"])})
    return m


@pytest.mark.parametrize("seed, max_conns, flow_logs", [(1, 0, False), (2, 9, True), (3, 5, False), (4, 0, True)])
def test_conversation_arrays_against_the_restatement_on_seeded_calls(nf, seed, max_conns, flow_logs):
    """The calls of test_conntrack_cpu's seeded mirror test. Every conversation record of the restatement, in its order, equals the
    row of the arrays decoded here; order names the flow a newConnection record precedes, and the record count for the others."""
    rng = np.random.default_rng(seed)
    ends = [("10.0.0.%d" % k, 1000 + k) for k in range(1, 8)] + [("2001:db8::%x" % k, 80 + 100 * k) for k in range(1, 8)]
    cfg = T.config(max_conns=max_conns, flow_logs=flow_logs)
    ref, mir = CT.ConnTrack(cfg), nf.ConnTrack(cfg)
    types = {v: k for k, v in nf._lib.CONN_RECORD_TYPES.items()}
    now, kinds, swapped = 0, set(), 0
    for call in range(9):
        flows = []
        for _ in range(40 if call < 8 else 0):
            fam = int(rng.integers(0, 2)) * 7
            a, b = rng.choice(7, 2, replace=bool(rng.integers(0, 8) == 0))
            flows.append(dict(src=ends[fam + a][0], sport=ends[fam + a][1], dst=ends[fam + b][0], dport=ends[fam + b][1],
                              proto=int(rng.choice([6, 6, 6, 17, 132, 1])), bytes=int(rng.integers(0, 1 << 40)) * int(rng.integers(0, 4) > 0),
                              packets=int(rng.integers(0, 1000)), flags=int(rng.choice([0, 0x10, 0x10, 0x11, 0x112, 0x01, 0x02]))))
        now += int(rng.integers(1, 4 * 10**9)) if call < 8 else 30 * 10**9
        recs = T.records(nf, flows)
        ms = T.maps(recs)
        want, at = [], []
        n_tracked = -1
        tracked = [i for i, m in enumerate(ms) if m.get(b"Proto") in (6, 17, 132)]
        for r in ref.extract(ms, now):
            if r[b"_RecordType"] == b"flowLog":
                n_tracked += 1
            else:
                want.append(r)
                at.append(len(recs) if r[b"_RecordType"] != b"newConnection" else tracked[n_tracked + 1] if flow_logs else None)
        parts = T.partial_array(nf, CT.fold(ms, T.KD)[0])
        car, val, order = mir.conversations(parts[rng.permutation(len(parts))], recs, now, T.NOW, T.MONO)
        assert len(car) == len(val) == len(order) == len(want) and (np.diff(order) >= 0).all()
        for j, r in enumerate(want):
            assert conv_of(T.FIELDS, car[j], val[j], types) == r, "call %d, record %d" % (call, j)
            if at[j] is not None:
                assert int(order[j]) == at[j]
            else:                                                    # without flow logs: the connection's first flow, found by its hash
                assert CT.compute_hash(ms[int(order[j])], T.KD)[2] == int(val[j]["hash_total"])
            swapped += r[b"SrcAddr"] != ms[int(order[j])][b"SrcAddr"] if r[b"_RecordType"] == b"newConnection" else 0
        kinds |= {r[b"_RecordType"] for r in want}
        assert len(mir) == len(ref.group_of)
    assert kinds == {b"newConnection", b"endConnection", b"heartbeat"} and swapped > 0
