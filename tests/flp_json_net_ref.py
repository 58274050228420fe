"""Independent restatement of three rules of flowlogs-pipeline's `transform network` stage over the maps of
tests/flp_json_k8s_ref.py, for the tests (no import of the product). Paths under flowlogs-pipeline's pkg/:

  pipeline/transform/transform_network_direction.go:32-64    reinterpretDirection
  pipeline/transform/transform_network.go:129-146,166-196    add_subnet_label, parseSubnets, applySubnetLabel
  pipeline/transform/transform_network.go:147-156            decode_tcp_flags, in place on Flags
  utils/tcp_flags.go:8-48                                    the flag table, DecodeTCPFlags
  Go's net.ParseCIDR, net.IP.Mask, net.IPNet.Contains        the family rules of a containment test

in the rule shape NetObserv configures: FlowDirectionField = FlowDirection, ReporterIPField = AgentIP, SrcHostField =
SrcK8S_HostIP, DstHostField = DstK8S_HostIP; SrcAddr -> SrcSubnetLabel, DstAddr -> DstSubnetLabel; Flags -> Flags. RecordToMap
writes no FlowDirection key, so the IfDirectionField copy (lines 33-35) never fires and is not restated. Rule order: add_kubernetes
src, dst, reinterpret_direction, add_kubernetes_infra, the two add_subnet_label, decode_tcp_flags. The two-minute ipLabelCache
cannot be seen between two configuration updates and is not restated.

Rules are a dict: direction (bool), labels (None: the rule is off; else [(name, [CIDR text])] in configuration order), flags
(bool)."""
import ipaddress
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_content_ref as RC  # noqa: E402
import flp_json_k8s_ref as K  # noqa: E402
import flp_json_tls_ref as RT  # noqa: E402
import netev_ref as RN  # noqa: E402
from flp_json_ref import go_ip, jsoniter_string, marshal_sorted, record_to_map  # noqa: E402

INGRESS, EGRESS, INNER = 0, 1, 2                      # transform_network_direction.go:12-16
TCP_FLAGS = ((1, b"FIN"), (2, b"SYN"), (4, b"RST"), (8, b"PSH"), (16, b"ACK"), (32, b"URG"), (64, b"ECE"), (128, b"CWR"),
             (256, b"SYN_ACK"), (512, b"FIN_ACK"), (1024, b"RST_ACK"))
V4_IN_V6 = bytes(10) + b"\xff\xff"
LABEL_MAX, MAX_CIDRS = 256, 1024
NO_LABEL, NO_DIRECTION = 0xFFFF, 0xFF
RULES_OFF = dict(direction=False, labels=None, flags=False)


def _b(v) -> bytes:
    return v.encode() if isinstance(v, str) else bytes(v)


def reinterpret_direction(out: dict) -> dict:
    """reinterpretDirection, lines 36-63."""
    reporter = out.get(b"AgentIP", b"")
    if not isinstance(reporter, bytes) or len(reporter) == 0:
        return out
    src = out.get(b"SrcK8S_HostIP", b"")
    dst = out.get(b"DstK8S_HostIP", b"")
    if src != dst:
        if src == reporter:
            out[b"FlowDirection"] = EGRESS
        elif dst == reporter:
            out[b"FlowDirection"] = INGRESS
    elif src != b"":
        out[b"FlowDirection"] = INNER
    return out


def cidr_mask(ones: int, bits: int) -> bytes:
    return (((1 << ones) - 1) << (bits - ones)).to_bytes(bits // 8, "big")


def ip_mask(ip: bytes, mask: bytes):
    """net.IP.Mask."""
    if len(mask) == 16 and len(ip) == 4 and mask[:12] == b"\xff" * 12:
        mask = mask[12:]
    if len(mask) == 4 and len(ip) == 16 and ip[:12] == V4_IN_V6:
        ip = ip[12:]
    if len(ip) != len(mask):
        return None
    return bytes(a & m for a, m in zip(ip, mask))


def parse_cidr(text: str):
    """net.ParseCIDR's *IPNet as (IP, Mask): the address as 16 bytes, a mask of the text's family, IP = addr16.Mask(m)."""
    addr, _, ones = text.partition("/")
    ip = ipaddress.ip_address(addr)
    n = int(ones)
    assert ones.isdigit() and 0 <= n <= ip.max_prefixlen
    m = cidr_mask(n, ip.max_prefixlen)
    addr16 = V4_IN_V6 + ip.packed if ip.version == 4 else ip.packed
    return ip_mask(addr16, m), m


def to4(ip: bytes):
    if len(ip) == 4:
        return ip
    if len(ip) == 16 and ip[:12] == V4_IN_V6:
        return ip[12:]
    return None


def contains(net_ip: bytes, mask: bytes, ip: bytes) -> bool:
    """net.IPNet.Contains with networkNumberAndMask."""
    nn = to4(net_ip)
    if nn is None:
        nn = net_ip
        if len(nn) != 16:
            return False
    m = mask
    if len(m) == 4:
        if len(nn) != 4:
            return False
    elif len(m) == 16:
        if len(nn) == 4:
            m = m[12:]
    else:
        return False
    x = to4(ip)
    if x is not None:
        ip = x
    if len(ip) != len(nn):
        return False
    return all(nn[k] & m[k] == ip[k] & m[k] for k in range(len(ip)))


def parse_subnets(categories):
    """parseSubnets: [(name bytes, [(IP, Mask)])], a category without CIDRs dropped."""
    cats = []
    for name, texts in categories:
        cidrs = [parse_cidr(t) for t in texts]
        if cidrs:
            cats.append((_b(name), cidrs))
    return cats


def parse_ip(text: bytes) -> bytes:
    """net.ParseIP of a text net.IP.String() printed: always the 16-byte form."""
    ip = ipaddress.ip_address(text.decode())
    return V4_IN_V6 + ip.packed if ip.version == 4 else ip.packed


def match_index(ip16: bytes, cats) -> int:
    """Index of the first category with a CIDR that contains the address, -1 for none (applySubnetLabel's walk)."""
    for c, (_, cidrs) in enumerate(cats):
        for net_ip, mask in cidrs:
            if contains(net_ip, mask, ip16):
                return c
    return -1


def apply_subnet_label(str_ip: bytes, cats) -> bytes:
    c = match_index(parse_ip(str_ip), cats)
    return cats[c][0] if c >= 0 else b""


def decode_tcp_flags(v: int):
    """DecodeTCPFlags: append to a nil slice, so no known bit leaves nil (jsoniter: null)."""
    names = [name for bit, name in TCP_FLAGS if v & bit]
    return names if names else None


def add_net(out: dict, rules: dict, cats) -> dict:
    """reinterpret_direction is applied by encode() between the Kubernetes rules; here the rules behind add_kubernetes_infra."""
    if rules.get("labels") is not None:
        for src, dst in ((b"SrcAddr", b"SrcSubnetLabel"), (b"DstAddr", b"DstSubnetLabel")):
            ip = out.get(src)
            if isinstance(ip, bytes):
                lbl = apply_subnet_label(ip, cats)
                if lbl != b"":
                    out[dst] = lbl
    if rules.get("flags"):
        if out.get(b"Flags") is not None:              # `ok && anyFlags != nil`; input == output: always written
            out[b"Flags"] = decode_tcp_flags(out[b"Flags"])
    return out


def apply_rules(m: dict, table: dict, layer, rules: dict, cats) -> dict:
    """The stage's rules on one flow's map, in their order."""
    K.enrich(m, b"SrcAddr", b"SrcK8S", table)
    K.enrich(m, b"DstAddr", b"DstK8S", table)
    if rules.get("direction"):
        reinterpret_direction(m)
    if layer is not None:
        K.enrich_layer(m, layer)
    return add_net(m, rules, cats)


def render(name, side: int) -> bytes:
    """One label's key as it stands in the sorted line, with its comma; nothing for an empty name."""
    name = _b(name)
    return b"," + jsoniter_string(b"DstSubnetLabel" if side else b"SrcSubnetLabel") + b":" + jsoniter_string(name) if name else b""


def encode(records, names_tls: dict, table: dict, layer, rules: dict, now_unix_ns, mono_now_ns, names, agent_ip, time_received,
           unknown=b"unknown", present=None, parts=None, events=None):
    """flp_json_k8s_ref.encode with all the stage's rules applied to each flow's map. Returns (bytes, offsets uint64[n + 1])."""
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1, 144)
    n = len(raw)
    off = np.zeros(n + 1, dtype=np.uint64)
    cats = parse_subnets(rules["labels"]) if rules.get("labels") is not None else []
    memo, lines, pos = {}, [], 0
    for i in range(n):
        rec = raw[i].tobytes()
        m = RT.add_tls(record_to_map(rec, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown, memo), rec, names_tls)
        if present is not None:
            RC.add_content(m, RC.flow_parts(present, parts, i))
        apply_rules(m, table, layer, rules, cats)
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


def resolve(records, entries, rules: dict, agent_ip) -> list:
    """[(src label, dst label, direction)] per record, as nfagg_net_resolve reports them: the index of the matched category
    among those that have CIDRs (NO_LABEL: none, or the rule is off), the direction (NO_DIRECTION: no key, or the rule is
    off). Plain dicts over the address bytes and the host-IP texts."""
    cats = parse_subnets(rules["labels"]) if rules.get("labels") is not None else []
    host = {K.ip16(ip): K._b(info.get("host_ip")) for ip, info in entries}
    reporter = go_ip(agent_ip)
    out = []
    for i in range(len(records)):
        is_ip = int(records["metrics"]["eth_protocol"][i]) in (0x0800, 0x86DD)
        sip, dip = records["id"]["src_ip"][i].tobytes(), records["id"]["dst_ip"][i].tobytes()
        lab = [NO_LABEL, NO_LABEL]
        if is_ip and rules.get("labels") is not None:
            for k, ip in enumerate((sip, dip)):
                c = match_index(ip, cats)
                lab[k] = c if c >= 0 else NO_LABEL
        d = NO_DIRECTION
        if rules.get("direction"):
            m = {b"AgentIP": reporter}
            if is_ip:
                for key, ip in ((b"SrcK8S_HostIP", sip), (b"DstK8S_HostIP", dip)):
                    if host.get(ip, b"") != b"":
                        m[key] = host[ip]
            d = reinterpret_direction(m).get(b"FlowDirection", NO_DIRECTION)
        out.append((lab[0], lab[1], d))
    return out
