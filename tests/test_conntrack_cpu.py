"""Conversation tracking, CPU side: the per-flow restatement of tests/conntrack_ref.py against the hand-worked vectors of
tests/golden/conntrack_vectors.json; nfagg_conn_hash (host, no handle) against the restatement; ConnTrack's Validate and
not-served errors; the layout of nfagg_conn_partial from a compiled C snippet; ConnTrack.apply fed hand-built partials (no
handle) against the restatement's output lists, exactly and in order."""
import ipaddress
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conntrack_ref as CT  # noqa: E402
import conntrack_streams as ST  # noqa: E402
import flp_json_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "conntrack_vectors.json")))
NOW, MONO = 1_700_000_000_123_456_789, 2_500_000_000_000
AGENT, RECEIVED = bytes(10) + b"\xff\xff" + bytes([10, 1, 2, 3]), 1_700_000_003
KD = {"fieldGroups": [{"name": "src", "fields": ["SrcAddr", "SrcPort"]}, {"name": "dst", "fields": ["DstAddr", "DstPort"]},
                      {"name": "common", "fields": ["Proto"]}],
      "hash": {"fieldGroupRefs": ["common"], "fieldGroupARef": "src", "fieldGroupBRef": "dst"}}
FIELDS = [dict(name="Bytes", operation="sum", splitAB=True), dict(name="Packets", operation="sum", splitAB=True),
          dict(name="numFlowLogs", operation="count"), dict(name="TimeFlowStart", operation="min", input="TimeFlowStartMs"),
          dict(name="TimeFlowEnd", operation="max", input="TimeFlowEndMs"), dict(name="FirstEtype", operation="first", input="Etype"),
          dict(name="LastDscp", operation="last", input="Dscp"), dict(name="FirstSrcMac", operation="first", input="SrcMac"),
          dict(name="LastIfDirections", operation="last", input="IfDirections")]
SCHEDULING = [dict(selector={"Proto": 17}, endConnectionTimeout="5s", terminatingTimeout="2s", heartbeatInterval="3s"),
              dict(selector={}, endConnectionTimeout="10s", terminatingTimeout="4s", heartbeatInterval="6s")]


def config(max_conns=0, flow_logs=False, no_new=False, **over):
    types = [t for t in ("newConnection", "endConnection", "heartbeat") if not (no_new and t == "newConnection")] + (["flowLog"] if flow_logs else [])
    c = dict(keyDefinition=json.loads(json.dumps(KD)), outputRecordTypes=types, outputFields=json.loads(json.dumps(FIELDS)),
             scheduling=json.loads(json.dumps(SCHEDULING)), maxConnectionsTracked=max_conns,
             tcpFlags=dict(fieldName="Flags", detectEndConnection=True, swapAB=True))
    c.update(over)
    return c


def ip16(text: str) -> bytes:
    a = ipaddress.ip_address(text)
    return bytes(10) + b"\xff\xff" + a.packed if a.version == 4 else a.packed


def records(nf, flows):
    """Vector flows -> 144-byte records: a dotted quad is an IPv4 record, anything else an IPv6 one (a "::ffff:" spelling too)."""
    r = np.zeros(len(flows), dtype=nf.FLOW_RECORD)
    for i, f in enumerate(flows):
        k, m = r[i]["id"], r[i]["metrics"]
        k["src_ip"], k["dst_ip"] = np.frombuffer(ip16(f["src"]), dtype=np.uint8), np.frombuffer(ip16(f["dst"]), dtype=np.uint8)
        k["src_port"], k["dst_port"], k["transport_protocol"] = f["sport"], f["dport"], f["proto"]
        m["eth_protocol"] = 0x86DD if ":" in f["src"] else 0x0800
        m["bytes"], m["packets"], m["flags"] = f.get("bytes", 0), f.get("packets", 0), f.get("flags", 0)
        m["start_mono_time_ts"], m["end_mono_time_ts"] = MONO - 7_000_000 * (i + 2), MONO - 3_000_000 * (i % 3)
        m["dscp"], m["if_index_first_seen"], m["direction_first_seen"] = i % 5, 2, i % 2
        m["src_mac"] = np.frombuffer(bytes([2, 0, 0, 0, 0, i % 7]), dtype=np.uint8)
    return r


def maps(recs, now=NOW, mono=MONO):
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 144)
    return [R.record_to_map(raw[i].tobytes(), now, mono, [], AGENT, RECEIVED) for i in range(len(raw))]


def norm(v):
    """The restatement's bytes as the product's text."""
    if isinstance(v, (bytes, bytearray)):
        return bytes(v).decode("latin-1")
    if isinstance(v, dict):
        return {norm(k): norm(x) for k, x in v.items()}
    if isinstance(v, list):
        return [norm(x) for x in v]
    return v


def partial_array(nf, parts):
    a = np.zeros(len(parts), dtype=nf.CONN_PARTIAL)
    for i, p in enumerate(parts):
        for k, v in p.items():
            a[i][k] = v
    return a


def summary(rec) -> str:
    ends = "%s:%d>%s:%d" % (rec["SrcAddr"], rec["SrcPort"], rec["DstAddr"], rec["DstPort"])
    if rec["_RecordType"] == "flowLog":
        return "flowLog " + ends
    return "%s %s n=%d ab=%d ba=%d first=%s" % (rec["_RecordType"], ends, rec.get("numFlowLogs", 0), rec.get("Bytes_AB", 0), rec.get("Bytes_BA", 0),
                                                   rec["_IsFirst"])


def trace_config(t):
    return config(max_conns=t.get("max_conns", 0), flow_logs=t.get("flow_logs", False), no_new=t.get("no_new", False))


# ---- the restatement against the vectors
@pytest.mark.parametrize("t", GOLDEN["tuples"], ids=[t["src_text"] + ">" + t["dst_text"] for t in GOLDEN["tuples"]])
def test_restatement_hashes_against_the_vectors(t):
    fl = {b"SrcAddr": t["src_text"].encode(), b"SrcPort": t["sport"], b"DstAddr": t["dst_text"].encode(), b"DstPort": t["dport"], b"Proto": t["proto"]}
    got = [CT.to_bytes(fl[k]).hex() for k in (b"SrcAddr", b"SrcPort", b"DstAddr", b"DstPort", b"Proto")]
    assert got == t["gob"]
    assert ["%x" % h for h in CT.compute_hash(fl, KD)] == [t["hash_a"], t["hash_b"], t["hash_total"]]
    back = {**fl, b"SrcAddr": fl[b"DstAddr"], b"SrcPort": fl[b"DstPort"], b"DstAddr": fl[b"SrcAddr"], b"DstPort": fl[b"SrcPort"]}
    a, b, total = CT.compute_hash(back, KD)
    assert ("%x" % total, "%x" % a, "%x" % b) == (t["hash_total"], t["hash_b"], t["hash_a"])      # equal for both directions
    assert len(GOLDEN["tuples"]) >= 12


def test_the_worked_gob_examples():
    assert CT.to_bytes(80).hex() == "03060050" and CT.to_bytes(443).hex() == "050600fe01bb" and CT.to_bytes(6).hex() == "03060006"
    assert CT.to_bytes(b"10.0.0.1").hex() == "0b0c000831302e302e302e31"
    assert CT.to_bytes(200).hex() == "040600ffc8" and CT.to_bytes(127).hex() == "0306007f" and CT.to_bytes(128).hex() == "040600ff80"


@pytest.mark.parametrize("t", GOLDEN["traces"], ids=[t["name"][:40] for t in GOLDEN["traces"]])
def test_restatement_against_the_traces(nf, t):
    ct = CT.ConnTrack(trace_config(t))
    for call in t["calls"]:
        got = [summary(norm(r)) for r in ct.extract(maps(records(nf, call["flows"])), call["now"])]
        assert got == call["want"], call
    assert len(GOLDEN["traces"]) >= 8


# ---- nfagg_conn_hash (host, no handle)
def test_conn_hash_against_the_vectors(nf):
    for t in GOLDEN["tuples"]:
        rec = records(nf, [t])[0]
        assert ["%x" % h for h in nf.conn_hash(rec.tobytes())] == [t["hash_total"], t["hash_a"], t["hash_b"]]
        assert norm(maps([rec])[0][b"SrcAddr"]) == t["src_text"]          # the restated net.IP.String() agrees with the vector's text
    other = records(nf, [dict(GOLDEN["tuples"][0], proto=1)])[0]
    assert nf.conn_hash(other.tobytes()) == (0, 0, 0)


def test_conn_hash_against_the_restatement_on_a_seeded_stream(nf):
    recs = ST.seeded_records(nf, 2000, 11)
    n_tracked = 0
    for rec, m in zip(recs, maps(recs)):
        tracked = b"Proto" in m and m[b"Proto"] in (6, 17, 132)
        a, b, total = CT.compute_hash(m, KD) if tracked else (0, 0, 0)
        assert nf.conn_hash(rec.tobytes()) == (total, a, b)
        n_tracked += tracked
    assert 400 < n_tracked < 1600          # v4, v6, non-IP and ICMP records are all there


# ---- Validate, and what this path does not serve
def _with(path, value):
    def f(c):
        d = c
        for k in path[:-1]:
            d = d[k]
        d[path[-1]] = value
    return f


VALIDATE = [
    (_with(["keyDefinition", "hash", "fieldGroupBRef"], ""), "only one of 'fieldGroupARef' and 'fieldGroupBRef' is set"),
    (_with(["outputFields", 2, "operation"], "avg"), "unknown operation 'avg'"),
    (_with(["outputFields", 5, "splitAB"], True), "unknown operation 'first'"),
    (_with(["outputFields", 1, "name"], "Bytes"), "duplicate outputField 'Bytes_AB'"),
    (lambda c: c["keyDefinition"]["fieldGroups"].append({"name": "src", "fields": []}), "duplicate fieldGroup 'src'"),
    (_with(["keyDefinition", "hash", "fieldGroupARef"], "nope"), "undefined fieldGroupARef 'nope'"),
    (_with(["keyDefinition", "hash", "fieldGroupBRef"], "nope"), "undefined fieldGroupBRef 'nope'"),
    (_with(["keyDefinition", "hash", "fieldGroupRefs"], ["common", "nope"]), "undefined fieldGroup 'nope'"),
    (_with(["outputRecordTypes"], ["newConnection", "update"]), "undefined output record type 'update'"),
    (_with(["scheduling", 0, "selector"], {"Dscp": 1}), "selector key 'Dscp' in scheduling group 0"),
    (_with(["scheduling", 0, "selector"], {}), "scheduling group 0 has a default selector but is not the last"),
    (_with(["scheduling", 1, "selector"], {"Proto": 6}), "found 0 default selectors"),
    (_with(["tcpFlags", "fieldName"], ""), "TCPFlags.FieldName is empty"),
    (lambda c: c["keyDefinition"]["fieldGroups"][0]["fields"].pop(), "mismatch between the field count"),
]


@pytest.mark.parametrize("change, message", VALIDATE, ids=[m[:30] for _, m in VALIDATE])
def test_validate_errors(nf, change, message):
    c = config()
    change(c)
    for make in (CT.ConnTrack, nf.ConnTrack):
        with pytest.raises(ValueError) as e:
            make(c)
        assert message in str(e.value)


def test_validate_errors_without_bidirection(nf):
    c = config()
    c["keyDefinition"]["hash"].update(fieldGroupARef="", fieldGroupBRef="")
    for make in (CT.ConnTrack, nf.ConnTrack):
        with pytest.raises(ValueError, match="has splitAB=true although bidirection is not enabled"):
            make(c)
    c["outputFields"] = [f for f in c["outputFields"] if not f.get("splitAB")]
    for make in (CT.ConnTrack, nf.ConnTrack):
        with pytest.raises(ValueError, match="SwapAB is enabled although bidirection is not enabled"):
            make(c)


NOT_SERVED = [
    (_with(["keyDefinition", "fieldGroups", 2, "fields"], ["Proto", "Dscp"]), "serves one key definition"),
    (_with(["keyDefinition", "hash", "fieldGroupRefs"], []), "serves one key definition"),
    (_with(["outputFields", 0, "input"], "DnsLatencyMs"), "sum over 'DnsLatencyMs' is not served"),
    (_with(["outputFields", 3, "input"], "Bytes"), "min is served over TimeFlowStartMs"),
    (_with(["outputFields", 4, "splitAB"], True), "max is served over TimeFlowEndMs, not split"),
    (_with(["outputFields", 5, "input"], "Flags"), "first over 'Flags'"),
    (_with(["outputFields", 6, "input"], "Interfaces"), "last over 'Interfaces'"),
    (_with(["outputFields", 0, "reportMissing"], True), "reportMissing on 'Bytes'"),
    (_with(["tcpFlags", "fieldName"], "TcpFlags"), "reads the record's Flags"),
]


@pytest.mark.parametrize("change, message", NOT_SERVED, ids=[m[:30] for _, m in NOT_SERVED])
def test_what_the_device_path_does_not_serve(nf, change, message):
    c = config()
    change(c)
    CT.ConnTrack(c)                                                      # Validate accepts it
    with pytest.raises(ValueError) as e:
        nf.ConnTrack(c)
    assert message in str(e.value)
    nf.ConnTrack(json.dumps(config()))                                   # JSON text is taken too


# ---- the layout of nfagg_conn_partial
PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "nfagg.h"
#define O(f) printf(#f " %zu\n", offsetof(nfagg_conn_partial, f))
int main(void){
 printf("size %zu\noptions %zu\n", sizeof(nfagg_conn_partial), sizeof(nfagg_conn_options));
 O(hash_total); O(first_hash_a); O(first_idx); O(last_idx); O(first_fin_idx); O(flags_or); O(flows); O(bytes); O(packets);
 O(start_ms_min); O(end_ms_max); O(pad_);
 printf("max %u\nno_idx %u\n", NFAGG_CONN_MAX_CONNS, NFAGG_CONN_NO_IDX);
 return 0; }
"""


def test_partial_layout_from_c(nf):
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src, "w").write(PROBE)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).strip().splitlines())}
    dt = nf.CONN_PARTIAL
    assert got.pop("size") == 128 == dt.itemsize and got.pop("options") == 24
    assert got.pop("max") == nf._lib.CONN_MAX_CONNS and got.pop("no_idx") == nf._lib.CONN_NO_IDX
    assert got == {name: dt.fields[name][1] for name in dt.names}
    assert [(n, getattr(nf._lib.ConnPartial, n).offset) for n in dt.names] == [(n, dt.fields[n][1]) for n in dt.names]


# ---- ConnTrack.apply on hand-built partials against the restatement
def run_both(nf, cfg, calls, rng=None):
    """calls: (now, vector flows). The mirror gets the restated fold's partials in a shuffled order; outputs must be equal."""
    ref, mir = CT.ConnTrack(cfg), nf.ConnTrack(cfg)
    outs = []
    for now, flows in calls:
        recs = records(nf, flows)
        ms = maps(recs)
        want = [norm(r) for r in ref.extract(ms, now)]
        parts, ids, _ = CT.fold(ms, KD)
        order = np.arange(len(parts)) if rng is None else rng.permutation(len(parts))
        got = mir.apply(partial_array(nf, parts)[order], recs, now, NOW, MONO, hash_ids=ids, flow_maps=[norm(m) for m in ms])
        assert got == want, "now = %d:\n got %r\nwant %r" % (now, got, want)
        assert len(mir) == len(ref.group_of)
        outs.append(got)
    return outs


@pytest.mark.parametrize("t", GOLDEN["traces"], ids=[t["name"][:40] for t in GOLDEN["traces"]])
def test_mirror_against_the_restatement_on_the_traces(nf, t):
    outs = run_both(nf, trace_config(t), [(c["now"], c["flows"]) for c in t["calls"]], np.random.default_rng(1))
    assert [[summary(r) for r in o] for o in outs] == [c["want"] for c in t["calls"]]


@pytest.mark.parametrize("seed, max_conns, flow_logs", [(1, 0, False), (2, 9, True), (3, 5, False), (4, 0, True)])
def test_mirror_against_the_restatement_on_seeded_calls(nf, seed, max_conns, flow_logs):
    """Eight calls of forty flows over fourteen endpoints: both directions, TCP / UDP / SCTP / ICMP, FIN and SYN_ACK at random,
    v4 and v6, the clock moving by up to four seconds, so that connections end by FIN, by timeout, reappear and beat."""
    rng = np.random.default_rng(seed)
    ends = [("10.0.0.%d" % k, 1000 + k) for k in range(1, 8)] + [("2001:db8::%x" % k, 80 + 100 * k) for k in range(1, 8)]
    calls, now = [], 0
    for _ in range(8):
        flows = []
        for _ in range(40):
            fam = int(rng.integers(0, 2)) * 7
            a, b = rng.choice(7, 2, replace=bool(rng.integers(0, 8) == 0))
            flows.append(dict(src=ends[fam + a][0], sport=ends[fam + a][1], dst=ends[fam + b][0], dport=ends[fam + b][1],
                              proto=int(rng.choice([6, 6, 6, 17, 132, 1])), bytes=int(rng.integers(0, 1 << 40)) * int(rng.integers(0, 4) > 0),
                              packets=int(rng.integers(0, 1000)), flags=int(rng.choice([0, 0x10, 0x10, 0x11, 0x112, 0x01, 0x02]))))
        now += int(rng.integers(1, 4 * 10**9))
        calls.append((now, flows))
    calls.append((now + 30 * 10**9, []))                                 # everything left ends
    outs = run_both(nf, config(max_conns=max_conns, flow_logs=flow_logs), calls, rng)
    kinds = {r["_RecordType"] for o in outs for r in o}
    assert {"newConnection", "endConnection", "heartbeat"} <= kinds
