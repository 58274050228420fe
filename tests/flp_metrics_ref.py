"""Independent restatement of flowlogs-pipeline's `encode prom` counters, per flow, over the enriched maps that
tests/flp_json_net_ref.apply_rules returns (no import of the product; it knows nothing of groups or classes). Paths under
flowlogs-pipeline's pkg/:

  pipeline/encode/metrics/preprocess.go:39-83     filterToPredicate, Preprocess
  pipeline/encode/metrics/filtering.go:5-35       ApplyFilters, applySingleFilter
  utils/filters/filters.go:13-148                 Presence, Absence, Equal, NotEqual, Regex, NotRegex, injectVars
  pipeline/encode/metrics_common.go:107-125       MetricCommonEncode's counter loop
  pipeline/encode/metrics_common.go:179-211       prepareMetric
  pipeline/encode/metrics_common.go:244-255       extractGenericValue
  pipeline/encode/metrics_common.go:265-295       extractLabels, newLabelKeyAndMap
  utils/convert.go:255-278                        ConvertToString
  api/encode_prom.go:49-79                        MetricsItem, MetricsFilter

Counters without `flatten` only (GenerateFlatParts then returns nothing and no filter uses flat parts). MaxMetrics and the expiry
cache (UpdateCacheEntry) are not restated: they depend on the order of the flows. Maps have bytes keys and bytes / int values, as
the other restatements build them; an item's keys, given as str, are encoded. Python's `re` stands in for Go's regexp."""
import re

VARIABLE = re.compile(rb"\$\(([^\)]+)\)")                      # filters.go:13


def _b(v) -> bytes:
    return v.encode() if isinstance(v, str) else bytes(v)


def convert_to_string(v) -> bytes:
    """ConvertToString, convert.go:255-278: integers in decimal (FormatInt / FormatUint, and %v for the narrow types), a string as it is."""
    if isinstance(v, bool):
        return b"true" if v else b"false"
    if isinstance(v, int):
        return b"%d" % v
    if isinstance(v, (bytes, bytearray)):
        return bytes(v)
    raise TypeError("not a value of the counters' keys: %r" % (v,))


def inject_vars(flow: dict, value: bytes, lookups) -> bytes:
    """injectVars, filters.go:134-148."""
    injected = value
    for whole, name in lookups:
        text = convert_to_string(flow[name]) if name in flow else b""          # :137-144: not found leaves ""
        injected = injected.replace(whole, text)                               # strings.ReplaceAll
    return injected


def equal(key: bytes, value: bytes):
    """Equal(key, value, true), filters.go:29-56."""
    lookups = [(m.group(0), m.group(1)) for m in VARIABLE.finditer(value)] if len(value) > 0 else []     # extractVarLookups :123-132
    if lookups:
        return lambda flow: key in flow and convert_to_string(flow[key]) == inject_vars(flow, value, lookups)   # :32-43
    return lambda flow: key in flow and convert_to_string(flow[key]) == value                                    # :46-55


def regex(key: bytes, pattern: bytes):
    """Regex, filters.go:105-116; MatchString searches anywhere in the text."""
    r = re.compile(pattern)
    return lambda flow: key in flow and r.search(convert_to_string(flow[key])) is not None


def filter_to_predicate(f: dict):
    """filterToPredicate, preprocess.go:39-58."""
    key, value, kind = _b(f["key"]), _b(f.get("value", "")), f.get("type", "")
    if kind == "equal":
        return equal(key, value)
    if kind == "not_equal":
        p = equal(key, value)                                                  # NotEqual, filters.go:65-68
        return lambda flow: not p(flow)
    if kind == "presence":
        return lambda flow: key in flow                                        # :15-20
    if kind == "absence":
        return lambda flow: key not in flow                                    # :22-27
    if kind == "match_regex":
        return regex(key, value)
    if kind == "not_match_regex":
        p = regex(key, value)                                                  # NotRegex :118-121
        return lambda flow: not p(flow)
    return equal(key, value)                                                   # "Default = Exact", :56-57


def preprocess(item: dict) -> dict:
    """Preprocess, preprocess.go:60-83, for an item without flatten."""
    assert not item.get("flatten")
    remap = item.get("remap") or {}
    labels = []
    for l in item.get("labels") or []:
        target = l
        if remap.get(l, "") != "":                                             # :67-69
            target = remap[l]
        labels.append((_b(l), target))
    filters = {}
    for f in item.get("filters") or []:                                        # :76-81
        filters.setdefault(f["key"], []).append(filter_to_predicate(f))
    return dict(name=item["name"], value_key=item.get("valueKey") or "", scale=float(item.get("valueScale") or 0), labels=labels, filters=filters)


def apply_filters(flow: dict, pre: dict) -> bool:
    """ApplyFilters, filtering.go:5-23: for a given key all filters are ORed; every key must pass."""
    for per_key in pre["filters"].values():
        all_failed = True
        for predicate in per_key:
            if predicate(flow):                                                # applySingleFilter :25-35, never flat
                all_failed = False
                break
        if all_failed:
            return False
    return True


def extract_generic_value(flow: dict, pre: dict):
    """extractGenericValue, metrics_common.go:244-255."""
    if pre["value_key"] == "":
        return 1
    return flow.get(_b(pre["value_key"]))                                      # not found: nil, the flow is skipped


def extract_labels(flow: dict, pre: dict) -> tuple:
    """extractLabels / newLabelKeyAndMap, metrics_common.go:265-295, no flat parts: ((target, value), ...) in label order."""
    out = []
    for source, target in pre["labels"]:
        value = b""
        if source in flow:
            value = convert_to_string(flow[source])
        out.append((target, value))
    return tuple(out)


class Counters:
    """MetricCommonEncode's counter loop with a CounterVec per item: values[(prefix + name, labels)] is what Add has summed, one
    float addition per flow."""

    def __init__(self, items, prefix: str = ""):
        self.pre = [preprocess(it) for it in items]
        self.prefix, self.values = prefix, {}

    def encode(self, flow: dict) -> None:
        for pre in self.pre:                                                   # metrics_common.go:111-125
            if not apply_filters(flow, pre):                                   # prepareMetric :180-184
                continue
            val = extract_generic_value(flow, pre)
            if val is None:                                                    # :186-189
                continue
            float_val = float(val)                                             # ConvertToFloat64
            if pre["scale"] != 0:                                              # :195-197
                float_val /= pre["scale"]
            key = (self.prefix + pre["name"], extract_labels(flow, pre))
            self.values[key] = self.values.get(key, 0.0) + float_val           # ProcessCounter: With(labels).Add(value)
