"""Independent restatement of flowlogs-pipeline's Kubernetes enrichment over the maps of tests/flp_json_tls_ref.py, for the
tests (no import of the product):

  pkg/pipeline/transform/kubernetes/enrich.go:37-104    Enrich: default assignee, no label / annotation prefixes, zone on
  pkg/pipeline/transform/kubernetes/enrich.go:140-165   EnrichLayer, objectIsApp
  pkg/api/transform_network.go:153-162                  the output key names

in the rule shape NetObserv configures: add_kubernetes for SrcAddr -> SrcK8S, for DstAddr -> DstK8S, then
add_kubernetes_infra -> K8S_FlowLayer over [(SrcK8S_Name, SrcK8S_Namespace), (DstK8S_Name, DstK8S_Namespace)].

The informers are not restated: their answers come as a table {address text as net.IP.String() prints it: info}, info a dict
with the byte strings namespace, name, kind, owner_name, owner_kind, network_name, host_ip, host_name (absent: empty) and zone
(None or absent: the node has no zone label; b"" is a label with an empty value). Enrich looks the record's SrcAddr / DstAddr
STRING up, as the reference does. A layer is (infra_prefixes, infra_refs), refs as (namespace, name) pairs."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_content_ref as RC  # noqa: E402
import flp_json_tls_ref as RT  # noqa: E402
import netev_ref as RN  # noqa: E402
from flp_json_ref import go_ip, jsoniter_string, marshal_sorted, record_to_map  # noqa: E402

FIELDS = ("namespace", "name", "kind", "owner_name", "owner_kind", "network_name", "host_ip", "host_name", "zone")
MAX_RENDERED = 2048
SEED_INDEX = 3          # ip_hash's seed index of the table (include/nfagg.h)
M64 = (1 << 64) - 1


def _b(v) -> bytes:
    return b"" if v is None else v.encode() if isinstance(v, str) else bytes(v)


def ip16(ip) -> bytes:
    """net.IP.To16() of 16 bytes, 4 bytes or dotted / colon text."""
    if isinstance(ip, str):
        import ipaddress
        ip = ipaddress.ip_address(ip).packed
    ip = bytes(ip)
    return bytes(10) + b"\xff\xff" + ip if len(ip) == 4 else ip


def table_of(entries) -> dict:
    """[(ip, info)] -> {address text: info with byte strings}."""
    out = {}
    for ip, info in entries:
        d = {f: _b(info.get(f)) for f in FIELDS[:-1]}
        d["zone"] = None if info.get("zone") is None else _b(info["zone"])
        out[go_ip(ip16(ip))] = d
    return out


def enrich(out: dict, ip_field: bytes, output: bytes, table: dict) -> dict:
    """Enrich (enrich.go:37-104) with rule.IPField / rule.Output."""
    ip = out.get(ip_field)
    if not isinstance(ip, bytes):                 # LookupString: no such key
        return out
    info = table.get(ip)
    if info is None:
        return out
    if info["namespace"] != b"":
        out[output + b"_Namespace"] = info["namespace"]
    out[output + b"_Name"] = info["name"]
    out[output + b"_Type"] = info["kind"]
    out[output + b"_OwnerName"] = info["owner_name"]
    out[output + b"_OwnerType"] = info["owner_kind"]
    out[output + b"_NetworkName"] = info["network_name"]
    if info["host_ip"] != b"":
        out[output + b"_HostIP"] = info["host_ip"]
        if info["host_name"] != b"":
            out[output + b"_HostName"] = info["host_name"]
    if info["zone"] is not None:                  # fillInK8sZone found the label
        out[output + b"_Zone"] = info["zone"]
    return out


def object_is_app(namespace: bytes, name: bytes, layer) -> bool:
    prefixes, refs = layer
    for p in prefixes:
        if namespace.startswith(_b(p)):
            return False
    for ns, nm in refs:
        if namespace == _b(ns) and name == _b(nm):
            return False
    return True


def enrich_layer(out: dict, layer) -> dict:
    """EnrichLayer (enrich.go:140-151)."""
    out[b"K8S_FlowLayer"] = b"infra"
    for name_f, ns_f in ((b"SrcK8S_Name", b"SrcK8S_Namespace"), (b"DstK8S_Name", b"DstK8S_Namespace")):
        ns = out.get(ns_f, b"")
        if ns != b"":
            if object_is_app(ns, out.get(name_f, b""), layer):
                out[b"K8S_FlowLayer"] = b"app"
                return out
    return out


def add_k8s(out: dict, table: dict, layer=None) -> dict:
    """The three rules in their order: src, dst, infra."""
    enrich(out, b"SrcAddr", b"SrcK8S", table)
    enrich(out, b"DstAddr", b"DstK8S", table)
    if layer is not None:
        enrich_layer(out, layer)
    return out


def render(ip, info: dict, side: int) -> bytes:
    """One side's keys as they stand in the sorted line, with the comma in front of each."""
    t = table_of([(ip, info)])
    text = next(iter(t))
    m = enrich({b"A": text}, b"A", b"DstK8S" if side else b"SrcK8S", t)
    del m[b"A"]
    return b"".join(b"," + jsoniter_string(k) + b":" + jsoniter_string(m[k]) for k in sorted(m))


def encode(records, names_tls: dict, table: dict, layer, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown=b"unknown",
           present=None, parts=None, events=None):
    """flp_json_tls_ref.encode with the three rules applied to each flow's map. Returns (bytes, offsets uint64[n + 1])."""
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1, 144)
    n = len(raw)
    off = np.zeros(n + 1, dtype=np.uint64)
    memo, lines, pos = {}, [], 0
    for i in range(n):
        rec = raw[i].tobytes()
        m = RT.add_tls(record_to_map(rec, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown, memo), rec, names_tls)
        if present is not None:
            RC.add_content(m, RC.flow_parts(present, parts, i))
        add_k8s(m, table, layer)
        body = marshal_sorted(m)
        if events is not None and events[i]:                # spliced in as netev_ref.encode_json does
            keys = sorted(list(m) + [b"NetworkEvents"])
            at = keys.index(b"NetworkEvents")
            val = b'"NetworkEvents":[' + b",".join(RN.render_json(e) for e in events[i]) + b"]"
            head = marshal_sorted({k: m[k] for k in keys[:at]})[:-1]
            tail = marshal_sorted({k: m[k] for k in keys[at + 1:]})[1:]
            body = head + (b"," if at else b"") + val + (b"," if len(tail) > 1 else b"") + tail
        lines.append(body + b"\n")
        pos += len(lines[-1])
        off[i + 1] = pos
    return b"".join(lines), off


def resolve(records, entries) -> np.ndarray:
    """uint32[n, 2]: the entry index of each record's src and dst address, 0xFFFFFFFF for none; a record that is not IP has
    no address key to look up. A plain dict over the 16 address bytes."""
    rows = {ip16(ip): r for r, (ip, _) in enumerate(entries)}
    out = np.full((len(records), 2), 0xFFFFFFFF, dtype=np.uint32)
    for i in range(len(records)):
        if int(records["metrics"]["eth_protocol"][i]) in (0x0800, 0x86DD):
            out[i, 0] = rows.get(records["id"]["src_ip"][i].tobytes(), 0xFFFFFFFF)
            out[i, 1] = rows.get(records["id"]["dst_ip"][i].tobytes(), 0xFFFFFFFF)
    return out


# ---- the table's hash (csrc/nfagg_hash.h: ip_hash with seed index 3), restated for crafting addresses by brute force
_SEEDS = (0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89)
_MUL = 0x9E3779B97F4A7C15


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _fmix(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    return x ^ (x >> 33)


def ip_hash(ip: bytes, seed_index: int = SEED_INDEX) -> int:
    lo, hi = int.from_bytes(ip[:8], "little"), int.from_bytes(ip[8:], "little")
    h = _SEEDS[seed_index & 3]
    h = ((_rotl(h, 27) ^ lo) * _MUL) & M64
    h = ((_rotl(h, 27) ^ hi) * _MUL) & M64
    return _fmix(h)


def capacity(n_rows: int) -> int:
    """Slots of a table of n_rows rows: the smallest power of two that leaves it at most half full."""
    cap = 1
    while cap < 2 * n_rows:
        cap <<= 1
    return cap


def craft(home: int, cap: int, count: int, make, start: int = 0):
    """`count` addresses make(k), k = start, start + 1, ..., whose home slot in a table of `cap` slots is `home`."""
    out, k = [], start
    while len(out) < count:
        ip = make(k)
        if ip_hash(ip) & (cap - 1) == home:
            out.append(ip)
        k += 1
    return out
