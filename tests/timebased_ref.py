"""flowlogs-pipeline's `extract timebased` restated structurally in Python, flow by flow, for the tests of nfagg_timebased_*:
a dict of lists of (stamp, flow map) per table (extract/timebased/tables.go), CalculateResults and CalculateValue
(filters.go:32-111), ComputeTopkBotk with a real binary heap (heap.go:62-157), CreateGenericMap (filters.go:167-191),
DeleteOldEntriesFromTables (tables.go:70-88), in the order of Extract (extract_timebased.go:35-59).

A flow map's keys may be str or bytes (tests/flp_json_ref.record_to_map writes bytes), its values int, float, str or bytes.
Time is integer nanoseconds. Go iterates its maps in random order; here a dict's insertion order stands in, so everything that
depends on that order (ties at the K-th place, the order of topK == 0) is unspecified and the tests compare accordingly.

ConvertToFloat64 of a missing key panics in the reference (utils/convert.go:56-59: reflect.Indirect of the zero Value, then
Type() on it); convert_to_float64(None) raises MissingKeyPanic."""
import math

MAX_FLOAT64 = 1.7976931348623157e308
OPERATIONS = ("sum", "avg", "min", "max", "count", "last", "diff")


class MissingKeyPanic(Exception):
    """reflect: call of reflect.Value.Type on zero Value."""


def get(entry: dict, key: str):
    if key in entry:
        return entry[key]
    return entry.get(key.encode())


def has(entry: dict, key: str) -> bool:
    return key in entry or key.encode() in entry


def convert_to_string(v) -> str:
    """utils.ConvertToString (convert.go:255-278) of the values a flow map holds."""
    if isinstance(v, (bytes, bytearray)):
        return bytes(v).decode("utf-8", "surrogateescape")
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, int):
        return "%d" % v
    if isinstance(v, float):
        return repr(v)
    return str(v)


def convert_to_float64(v) -> float:
    """utils.ConvertToFloat64 (convert.go:36-69)."""
    if v is None:
        raise MissingKeyPanic("reflect: call of reflect.Value.Type on zero Value")
    if isinstance(v, (bytes, bytearray)):
        return float(bytes(v).decode())
    return float(v)


def init_value(op: str) -> float:
    return -MAX_FLOAT64 if op == "max" else MAX_FLOAT64 if op == "min" else 0.0


class _Item:
    """A heap item under one of the two Less functions of heap.go."""

    def __init__(self, value, key, bottom):
        self.value, self.key, self.bottom = value, key, bottom

    def less(self, other) -> bool:
        return self.value > other.value if self.bottom else self.value < other.value


def _up(h, j):
    while True:
        i = (j - 1) // 2
        if i == j or j <= 0 or not h[j].less(h[i]):
            break
        h[i], h[j] = h[j], h[i]
        j = i


def _down(h, i0, n):
    i = i0
    while True:
        j1 = 2 * i + 1
        if j1 >= n or j1 < 0:
            break
        j = j1
        if j1 + 1 < n and h[j1 + 1].less(h[j1]):
            j = j1 + 1
        if not h[j].less(h[i]):
            break
        h[i], h[j] = h[j], h[i]
        i = j


def heap_push(h, x):
    h.append(x)
    _up(h, len(h) - 1)


def heap_pop(h):
    n = len(h) - 1
    h[0], h[n] = h[n], h[0]
    _down(h, 0, n)
    return h.pop()


def top_or_bottom_k(results: dict, k: int, bottom: bool) -> list:
    """computeTopK / computeBotK: [(key, value)], the best first."""
    prev = MAX_FLOAT64 if bottom else -MAX_FLOAT64
    h = []
    for key, val in results.items():
        if (val > prev) if bottom else (val < prev):
            continue
        heap_push(h, _Item(val, key, bottom))
        if len(h) > k:
            prev = heap_pop(h).value
    out = [None] * len(h)
    for i in range(len(h), 0, -1):
        it = heap_pop(h)
        out[i - 1] = (it.key, it.value)
    return out


class Timebased:
    """The stage. rules: the api.TimebasedFilterRule dicts (name, indexKey / indexKeys, operationType, operationKey, topK,
    reversed, timeInterval in ns). extract(entries, now) -> the maps; `filters[i]["results"]` is rule i's full Results map."""

    def __init__(self, rules):
        self.tables, self.filters, self.skipped = {}, [], []
        for ru in rules:
            ru = dict(ru)
            keys = list(ru.get("indexKeys") or [])
            if keys:
                ru["indexKey"] = ",".join(keys)
            elif ru.get("indexKey"):
                keys = [ru["indexKey"]]
            else:
                self.skipped.append(ru)
                continue
            ru["indexKeys"] = keys
            interval = int(ru.get("timeInterval") or 0)
            t = self.tables.get(ru["indexKey"])
            if t is None:
                t = self.tables[ru["indexKey"]] = dict(max_interval=interval, data={})
            elif interval > t["max_interval"]:
                t["max_interval"] = interval
            if ru.get("operationType") not in OPERATIONS:
                self.skipped.append(ru)
                continue
            self.filters.append(dict(rule=ru, table=t, results={}, output=[]))

    def add_entry(self, entry: dict, now: int) -> None:
        for table_key, t in self.tables.items():
            keys = table_key.split(",")
            valid, parts = 0, []
            for key in keys:
                if has(entry, key):
                    s = convert_to_string(get(entry, key))
                    if len(s) > 0:
                        parts.append(s)
                        valid += 1
            if valid == len(keys):
                t["data"].setdefault(",".join(parts), []).append((now, entry))

    def calculate_results(self, f, now: int) -> None:
        ru = f["rule"]
        oldest = now - int(ru.get("timeInterval") or 0)
        op, opkey = ru["operationType"], ru.get("operationKey", "")
        for table_key, l in f["table"]["data"].items():
            value = 0.0
            if op == "last":
                if not l:
                    continue
                value = convert_to_float64(get(l[-1][1], opkey))
            elif op == "diff":
                for stamp, entry in l:
                    if stamp < oldest:
                        continue
                    first = convert_to_float64(get(entry, opkey))
                    last = convert_to_float64(get(l[-1][1], opkey))
                    value = last - first
                    break
            else:
                value, n = init_value(op), 0
                for stamp, entry in l:
                    if stamp < oldest:
                        continue
                    v = convert_to_float64(get(entry, opkey))
                    n += 1
                    if op in ("sum", "avg"):
                        value += v
                    elif op == "max":
                        value = max(value, v)
                    elif op == "min":
                        value = min(value, v)
                if op == "avg" and n > 0:
                    value /= float(n)
                if op == "count":
                    value = float(n)
            f["results"][table_key] = value

    def output_of(self, f) -> list:
        ru = f["rule"]
        k = int(ru.get("topK") or 0)
        if k > 0:
            return top_or_bottom_k(f["results"], k, bool(ru.get("reversed")))
        return list(f["results"].items())

    def generic_maps(self, f) -> list:
        ru, out = f["rule"], []
        for key, value in f["output"]:
            m = {"name": ru.get("name", ""), "index_key": ru["indexKey"], "operation": ru["operationType"]}
            m[ru.get("operationKey", "")] = value
            values = key.split(",")
            if len(values) == len(ru["indexKeys"]):
                for i, k in enumerate(ru["indexKeys"]):
                    m[k] = values[i]
            out.append(m)
        return out

    def delete_old(self, now: int) -> None:
        for t in self.tables.values():
            oldest = now - t["max_interval"]
            for l in t["data"].values():
                while l and l[0][0] < oldest:
                    l.pop(0)

    def extract(self, entries, now: int) -> list:
        for e in entries:
            self.add_entry(e, now)
        out = []
        self.per_rule = []
        for f in self.filters:
            self.calculate_results(f, now)
            f["output"] = self.output_of(f)
            maps = self.generic_maps(f)
            self.per_rule.append(maps)
            out.extend(maps)
        self.delete_old(now)
        return out


def same_bits(a: float, b: float) -> bool:
    """== on float64, and the sign of zero."""
    import struct
    return a == b and struct.pack("<d", a) == struct.pack("<d", b) and not math.isnan(a)
