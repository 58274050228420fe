"""extract conntrack's conversation records as the JSON lines a flowlogs-pipeline writes, restated without the product:
conn.go:101-114 (toGenericMap: aggregates as float64, omitted when zero; first / last values, a nil omitted; the keys prevail),
addHashField / addTypeField / addIsFirstField (conntrack.go:281-295), the transform network rules that key off the addresses
(tests/flp_json_net_ref.apply_rules; reinterpret_direction returns at once, a conversation has no AgentIP), then
jsoniter.Config{SortMapKeys: true}.Marshal: flp_json_ref.marshal_sorted extended by float64 values and booleans.

float64: jsoniter's WriteFloat64 (stream_float.go:65-79) prints with strconv format 'f', precision -1, below 1e21. For an integer
of magnitude below 2^53 that is its decimal digits. Above, the shortest round-trip digits are padded with zeros, which this file
does not print: marshal() raises Deferred, and the record must be deferred by the encoder under test. What the host then
writes for such a record is float_f(), which marshal(m, defer=False) uses.

The expected lines are pinned to this restatement and to jsoniter's source, not to a Go run."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_net_ref as R  # noqa: E402
from flp_json_ref import jsoniter_string  # noqa: E402

EXACT = 1 << 53
KEYS = (b"SrcAddr", b"DstAddr", b"SrcPort", b"DstPort", b"Proto")


class Deferred(ValueError):
    pass


def float_f(v: float) -> bytes:
    """strconv.FormatFloat(v, 'f', -1, 64) of an integral float64 of magnitude below 1e21: the fewest digits that read back as v
    (found by trying 1 to 17 with the C library's correctly rounded %e), then zeros up to the decimal point."""
    assert v == int(v) and abs(v) < 1e21
    for p in range(1, 18):
        mant, exp = (b"%.*e" % (p - 1, abs(v))).split(b"e")
        if float(mant + b"e" + exp) == abs(v):
            digits = mant.replace(b".", b"")
            assert int(exp) + 1 >= len(digits)
            return (b"-" if v < 0 else b"") + digits + b"0" * (int(exp) + 1 - len(digits))
    raise AssertionError(v)


def _value(v, defer=True) -> bytes:
    if v is None:
        return b"null"
    if isinstance(v, bool):
        return b"true" if v else b"false"
    if isinstance(v, float):
        if (defer and abs(v) >= EXACT) or v != v or abs(v) == float("inf") or v != int(v):
            raise Deferred(repr(v))
        return str(int(v)).encode() if abs(v) < EXACT else float_f(v)
    if isinstance(v, (bytes, bytearray)):
        return jsoniter_string(bytes(v))
    if isinstance(v, list):
        return b"[" + b",".join(_value(x) for x in v) + b"]"
    return str(int(v)).encode()


def marshal(m: dict, defer=True) -> bytes:
    """defer: raise Deferred for a float64 of magnitude >= 2^53 (what the device encoder must do); False prints it with float_f."""
    return b"{" + b",".join(jsoniter_string(k) + b":" + _value(m[k], defer) for k in sorted(m)) + b"}"


def to_map(fields, conv: dict) -> dict:
    """conn.go:101-114. fields: the stage's outputFields; conv: keys (the five), flows / bytes / packets as (AB, BA) integers,
    start_min, end_max, first / last: {input name: value}."""
    gm = {}
    for f in fields:
        op, name = f["operation"], f["name"].encode() if isinstance(f["name"], str) else f["name"]
        inp = f.get("input", "") or f["name"]
        if op in ("first", "last"):
            v = conv[op].get(inp)
            if v is not None:
                gm[name] = v
            continue
        if op == "min":
            vals = [(name, conv["start_min"])]
        elif op == "max":
            vals = [(name, conv["end_max"])]
        else:
            ab, ba = conv["flows"] if op == "count" else conv["bytes"] if inp == "Bytes" else conv["packets"]
            vals = [(name + b"_AB", ab), (name + b"_BA", ba)] if f.get("splitAB", False) else [(name, ab + ba)]
        for k, v in vals:
            if abs(v) >= EXACT:                   # a float64 would round it: not restated here
                gm[k] = float("inf")
            elif v != 0:
                gm[k] = float(v)
    gm.update(conv["keys"])
    return gm


def record(fields, conv: dict, table: dict, layer, rules: dict, cats) -> dict:
    m = to_map(fields, conv)
    m[b"_HashId"] = b"%x" % conv["hash"]
    m[b"_RecordType"] = conv["type"]
    m[b"_IsFirst"] = bool(conv["is_first"])
    return R.apply_rules(m, table, layer, rules, cats)


def line(fields, conv, table, layer, rules, cats) -> bytes:
    """The conversation's line with its newline; raises Deferred for a record the device must defer."""
    return marshal(record(fields, conv, table, layer, rules, cats)) + b"\n"
