"""Independent per-flow restatement of flowlogs-pipeline's `transform filter` stage over the enriched maps of the other
restatements (flp_json_ref.record_to_map plus what flp_json_content_ref, flp_json_k8s_ref and flp_json_net_ref add), for the
tests. It walks a parsed query tree with the rules of utils/filters/filters.go and utils/convert.go, applies the rules in
transform_filter.go's order, and rolls with the documented counter-based roll. It knows nothing of atoms, ops or steps beyond
the numbering of the steps, which the roll takes. Paths under flowlogs-pipeline's pkg/:

  pipeline/transform/transform_filter.go:55-95     Transform: the keep rules first, then the others in order
  pipeline/transform/transform_filter.go:99-122    the four remove_entry_* rules (interface{} == / !=)
  pipeline/transform/transform_filter.go:168-215   remove_entry_all_satisfied, conditional_sampling, applyKeepPredicate
  pipeline/transform/transform_filter.go:217-232   rollSampling, storeSampling
  utils/filters/filters.go:15-121                  Presence, Absence, Equal (convertString false), the numeric six, Regex
  utils/convert.go:178-213                         ConvertToInt
  dsl/eval.go:14-33                                and / or over the tree

Maps hold Go's types apart: bytes for a string, int for every integer type, list for a slice, None for a nil slice. A tree is
what the product's parse_query returns: ("and" | "or", l, r), ("with" | "without", key), ("cmp", key, op, value)."""
import re

K = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
NO_RULE = 0xFF
_INT = re.compile(rb"[+-]?[0-9]+\Z")


def fmix64(x: int) -> int:
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M64
    return x ^ (x >> 33)


def roll(seed: int, flow_index: int, step: int, value: int) -> bool:
    """include/nfagg.h, nfagg_filter_roll."""
    if value == 0:
        return True
    return fmix64(fmix64((seed + K * flow_index) & M64) ^ (K * (step + 1) & M64)) % value == 0


def convert_to_int(v):
    """ConvertToInt: (int, ok). Every integer type converts, a uint64 wraps; a string goes through ParseInt; a slice fails."""
    if isinstance(v, bool) or v is None or isinstance(v, list):
        return 0, False
    if isinstance(v, int):
        v &= M64
        return (v - (1 << 64) if v >= 1 << 63 else v), True
    if isinstance(v, bytes):
        if not _INT.match(v):
            return 0, False
        x = int(v)
        return (x, True) if -(1 << 63) <= x < (1 << 63) else (0, False)
    return 0, False


def convert_to_string(v) -> bytes:
    """ConvertToString of the values these maps hold (fmt's %v for a slice)."""
    if isinstance(v, bytes):
        return v
    if isinstance(v, int):
        return b"%d" % v
    if v is None:
        return b"[]"
    return b"[" + b" ".join(convert_to_string(x) for x in v) + b"]"


def evaluate(tree, m: dict) -> bool:
    kind = tree[0]
    if kind == "and":
        return evaluate(tree[1], m) and evaluate(tree[2], m)
    if kind == "or":
        return evaluate(tree[1], m) or evaluate(tree[2], m)
    key = tree[1].encode()
    if kind == "with":
        return key in m
    if kind == "without":
        return key not in m
    op, value = tree[2], tree[3]
    found = key in m
    if op in ("=~", "!~"):
        hit = found and re.search(value, convert_to_string(m[key])) is not None
        return hit if op == "=~" else not hit
    if isinstance(value, bytes):                                     # Equal / NotEqual with convertString false: val == filterValue
        hit = found and isinstance(m[key], bytes) and m[key] == value
        return hit if op == "=" else not hit
    if not found:
        return False
    x, ok = convert_to_int(m[key])
    if not ok:
        return False
    return {"=": x == value, "!=": x != value, "<": x < value, ">": x > value, "<=": x <= value, ">=": x >= value}[op]


def _go_equal(val, value) -> bool:
    """interface{} == between a map value and a rule's YAML value: a string equals an equal string; a YAML number (int or
    float64) never equals the uint8 / uint16 / uint32 / uint64 / int64 a flow's map holds."""
    return isinstance(val, bytes) and isinstance(value, (str, bytes)) and val == (value.encode() if isinstance(value, str) else value)


def remove_entry(t: str, g: dict, m: dict) -> bool:
    """True when the rule removes the flow (applyRule returns false)."""
    key = (g.get("input") or "").encode()
    if t == "remove_entry_if_exists":
        return key in m
    if t == "remove_entry_if_doesnt_exist":
        return key not in m
    if t == "remove_entry_if_equal":
        return key in m and _go_equal(m[key], g.get("value"))
    if t == "remove_entry_if_not_equal":
        return key in m and not _go_equal(m[key], g.get("value"))
    raise ValueError(t)


def all_satisfied(rules, m: dict) -> bool:
    return all(remove_entry(r["type"], r.get("removeEntry") or {}, m) for r in rules)


def transform(cfg: dict, m: dict, parse, seed: int, flow_index: int):
    """One flow: (keep, rule, map). keep 0: dropped (map None); 1: kept; 2: kept, and the stored Sampling does not fit 32 bits.
    rule: the admitting keep rule's step, NO_RULE if none. Steps are numbered as the product lays them out: the keep rules in
    configuration order, then one per other rule, a conditional_sampling rule taking one per condition."""
    out = dict(m)
    rules = cfg.get("rules") or []
    keeps = [r for r in rules if r.get("type") == "keep_entry_query"]
    others = [r for r in rules if r.get("type") != "keep_entry_query"]
    admit, deferred = NO_RULE, False
    if keeps:
        for s, r in enumerate(keeps):
            if evaluate(parse(r["keepEntryQuery"]), out):
                value = int(r.get("keepEntrySampling") or 0)
                if value > 0:
                    if not roll(seed, flow_index, s, value):
                        continue                                     # sampled out of this rule: the next one is still tried
                    if cfg.get("samplingField"):
                        cur = out.get(b"Sampling", 1)                # storeSampling
                        out[b"Sampling"] = (cur if cur else 1) * value
                        deferred = out[b"Sampling"] > 0xFFFFFFFF
                admit = s
                break
        if admit == NO_RULE:
            return 0, NO_RULE, None
    step = len(keeps)
    for r in others:
        t = r.get("type")
        if t == "remove_entry_all_satisfied":
            if all_satisfied(r.get("removeEntryAllSatisfied") or [], out):
                return 0, admit, None
            step += 1
        elif t == "conditional_sampling":
            conds = r.get("conditionalSampling") or []
            for k, c in enumerate(conds):
                if all_satisfied(c.get("rules") or [], out):
                    if not roll(seed, flow_index, step + k, int(c.get("value") or 0)):
                        return 0, admit, None
                    break
            step += len(conds)
        else:
            if remove_entry(t, r.get("removeEntry") or {}, out):
                return 0, admit, None
            step += 1
    return (2 if deferred else 1), admit, out


def run(cfg: dict, maps, parse, seed: int = 0, first_index: int = 0):
    """The stage over a batch: (keep list, rule list, kept indexes, kept maps)."""
    memo = {}
    cached = lambda text: memo[text] if text in memo else memo.setdefault(text, parse(text))  # noqa: E731
    keep, rule, idx, kept = [], [], [], []
    for i, m in enumerate(maps):
        k, r, out = transform(cfg, m, cached, seed, first_index + i)
        keep.append(k)
        rule.append(r)
        if k:
            idx.append(i)
            kept.append(out)
    return keep, rule, idx, kept


def light_maps(recs, net_rows=None):
    """The numeric keys of decode_protobuf.go:63-128 straight from the record columns (no interface names, no texts), for the
    big batches: Etype, Bytes, Packets, Sampling, Proto, Dscp, SrcPort, DstPort, IcmpType, IcmpCode, Flags; FlowDirection from
    net_rows where given."""
    cols = {k: recs["metrics"][k].tolist() for k in ("eth_protocol", "bytes", "packets", "sampling", "dscp", "flags")}
    ids = {k: recs["id"][k].tolist() for k in ("transport_protocol", "src_port", "dst_port", "icmp_type", "icmp_code")}
    dirs = net_rows["direction"].tolist() if net_rows is not None else None
    maps = []
    for i in range(len(recs)):
        eth, proto = cols["eth_protocol"][i], ids["transport_protocol"][i]
        m = {b"Etype": eth, b"SrcMac": b"", b"DstMac": b""}
        for key, col in ((b"Bytes", "bytes"), (b"Packets", "packets"), (b"Sampling", "sampling")):
            if cols[col][i]:
                m[key] = cols[col][i]
        if eth in (0x0800, 0x86DD):
            m[b"Proto"], m[b"Dscp"] = proto, cols["dscp"][i]
            if proto in (1, 58):
                m[b"IcmpType"], m[b"IcmpCode"] = ids["icmp_type"][i], ids["icmp_code"][i]
            elif proto in (6, 17, 132):
                m[b"SrcPort"], m[b"DstPort"] = ids["src_port"][i], ids["dst_port"][i]
                if proto == 6:
                    m[b"Flags"] = cols["flags"][i]
        if dirs is not None and dirs[i] <= 2:
            m[b"FlowDirection"] = dirs[i]
        maps.append(m)
    return maps
