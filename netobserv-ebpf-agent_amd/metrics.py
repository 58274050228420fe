"""The counters and histograms of flowlogs-pipeline's `encode prom` stage over the GPU's grouped sums (nfagg_metrics_fold,
nfagg_metrics_fold_content): the host mirror of pkg/pipeline/encode/metrics_common.go:107-125,144-159,179-211,265-295 that
visits the GROUPS, not the flows.

The reference runs prepareMetric for every flow and every metric: filters, value key, label map, cache lookup, Add. Here the
device groups the flows by the keys a metric's labels and filters name and sums flows, bytes and packets; per group this module
rebuilds those keys, applies the filters (ApplyFilters, encode/metrics/filtering.go:5-23, over the six predicates of
utils/filters/filters.go), takes the value and the labels and adds once. That is exact: every predicate and every label value
is a function of the grouping's keys alone.

Strings are bytes throughout, as Go's are: keys and label targets are str, values (label values, filter values after UTF-8
encoding) are bytes. Python's `re` stands in for Go's RE2 (regexp.MatchString is an unanchored search: re.search); the two
engines agree on the common syntax, but not on everything (RE2 has no backreferences or lookaround; a few escapes differ), so a
pattern that only one of them accepts, or that they read differently, is the caller's to avoid.

PromCounters serves counters over the record's own keys. PromMetrics serves counters and histograms, and adds the keys of a
MapTracer flow's feature parts: the values TimeFlowRttNs, DnsLatencyMs, PktDropBytes and PktDropPackets, the labels
DnsFlagsResponseCode, PktDropLatestDropCause, PktDropLatestState and IPSecStatus. A histogram is a GROUP BY over (keys, bucket):
the device compares integers, so every float bound becomes the largest integer of the value's domain that the reference's own
float arithmetic (float64(x) / valueScale <= bound) still accepts. That is exact, because float64(x) / scale does not decrease
with x. The vendored FLP registers its histograms without Buckets (encode_prom.go:130-134), so prometheus.DefBuckets apply
whatever the item says; item_buckets=True takes the item's list, as newer FLP does.

Not restated, by design: MaxMetrics and the expiry cache (order-dependent, the caller's business), gauges (last write wins),
agg_histogram, `flatten`, and keys outside the two dimension lists (Interfaces, Dscp, DnsName, ...): the classes raise ValueError
for such an item, which stays on the host path."""
import re


from . import _lib as L
from .table import K8S_FIELDS, flp_enum_name

K8S_SUFFIXES = ("Namespace", "Name", "Type", "OwnerName", "OwnerType", "NetworkName", "HostIP", "HostName", "Zone")   # transform_network.go:153-162
KEY_DIMS = {}
for _f, _s in enumerate(K8S_SUFFIXES):
    KEY_DIMS["SrcK8S_" + _s] = L.DIM_SRC_K8S(_f)
    KEY_DIMS["DstK8S_" + _s] = L.DIM_DST_K8S(_f)
KEY_DIMS.update(SrcSubnetLabel=L.DIM_SRC_SUBNET_LABEL, DstSubnetLabel=L.DIM_DST_SUBNET_LABEL, FlowDirection=L.DIM_FLOW_DIRECTION,
                K8S_FlowLayer=L.DIM_FLOW_LAYER, Proto=L.DIM_PROTO)
NET_DIMS = L.DIM_SRC_SUBNET_LABEL | L.DIM_DST_SUBNET_LABEL | L.DIM_FLOW_DIRECTION
VALUE_FIELDS = {"": ("flows", "flows"), "Bytes": ("bytes", "flows_with_bytes"), "Packets": ("packets", "flows_with_packets")}
VARIABLE = re.compile(rb"\$\(([^\)]+)\)")                 # filters.go:13
FILTER_TYPES = ("equal", "not_equal", "presence", "absence", "match_regex", "not_match_regex")      # api/encode_prom.go:65-73


def _b(v) -> bytes:
    return v.encode() if isinstance(v, str) else bytes(v)


def convert_to_string(v) -> bytes:
    """utils.ConvertToString (utils/convert.go:255-278) of the values a group's keys take: strings and small integers."""
    return b"%d" % v if isinstance(v, int) else bytes(v)


def _field_present(info: dict, f: int) -> bool:
    """nfagg_k8s_render's presence of K8S_FIELDS[f] (enrich.go:51-87)."""
    name = K8S_FIELDS[f]
    if name in ("namespace", "host_ip"):
        return len(_b(info.get(name) or b"")) != 0
    if name == "host_name":
        return len(_b(info.get("host_ip") or b"")) != 0 and len(_b(info.get("host_name") or b"")) != 0
    if name == "zone":
        return info.get("zone") is not None
    return True


def group_keys(dims: int, group, entries, labels, class_row, g: int) -> dict:
    """The grouping's keys of one group as the enriched map holds them: {key: bytes or int}, an absent key left out. entries:
    the Kubernetes table's [(ip, info)]; labels: the net table's label texts; class_row(g, side, cls) -> entry index."""
    m = {}
    for side, prefix, cls in ((0, "SrcK8S_", int(group["src_class"])), (1, "DstK8S_", int(group["dst_class"]))):
        sel = (dims >> (9 * side)) & 0x1FF
        if not sel or not cls:
            continue
        info = entries[class_row(g, side, cls)][1]
        for f in range(9):
            if sel >> f & 1 and _field_present(info, f):
                m[prefix + K8S_SUFFIXES[f]] = _b(info.get(K8S_FIELDS[f]) or b"")
    for key, field, dim in (("SrcSubnetLabel", "src_label", L.DIM_SRC_SUBNET_LABEL), ("DstSubnetLabel", "dst_label", L.DIM_DST_SUBNET_LABEL)):
        k = int(group[field]) if dims & dim else L.NET_NO_LABEL
        if k != L.NET_NO_LABEL and labels[k]:                            # an empty name ends the search and writes no key
            m[key] = _b(labels[k])
    if dims & L.DIM_FLOW_DIRECTION and int(group["direction"]) != L.NET_NO_DIRECTION:
        m["FlowDirection"] = int(group["direction"])
    if dims & L.DIM_FLOW_LAYER and int(group["layer"]):
        m["K8S_FlowLayer"] = b"app" if int(group["layer"]) == 2 else b"infra"
    if dims & L.DIM_PROTO and int(group["is_ip"]):
        m["Proto"] = int(group["proto"])
    return m


class _Filter:
    """One MetricsFilter as filterToPredicate builds it (encode/metrics/preprocess.go:39-58)."""

    def __init__(self, f: dict):
        self.key, self.type = f["key"], f.get("type") or "equal"
        self.value = _b(f.get("value", ""))
        if self.type not in FILTER_TYPES:
            self.type = "equal"                                          # "Default = Exact"
        self.vars = [(m.group(0), m.group(1).decode()) for m in VARIABLE.finditer(self.value)] if self.type in ("equal", "not_equal") else []
        self.regex = re.compile(self.value) if self.type in ("match_regex", "not_match_regex") else None

    def keys(self):
        return [self.key] + [name for _, name in self.vars]

    def __call__(self, m: dict) -> bool:
        found = self.key in m
        if self.type == "presence":
            return found
        if self.type == "absence":
            return not found
        if self.type in ("equal", "not_equal"):
            want = self.value
            for text, name in self.vars:                                 # injectVars: a missing key injects ""
                want = want.replace(text, convert_to_string(m[name]) if name in m else b"")
            hit = found and convert_to_string(m[self.key]) == want
            return hit if self.type == "equal" else not hit
        hit = found and self.regex.search(convert_to_string(m[self.key])) is not None
        return hit if self.type == "match_regex" else not hit


class PromCounters:
    """`encode prom` counters fed by the GPU fold. items: FLP MetricsItem dicts (api/encode_prom.go:49-60: name, type, filters,
    valueKey, labels, remap, flatten, valueScale). Each item's grouping is the set of keys its labels and filters (and the
    $(Key) variables of its equal filters) name; equal groupings are shared. ValueError for an item this path cannot serve: a
    type other than counter, `flatten`, a value key other than "" / Bytes / Packets, a label or filter key outside the
    dimension list, more than L.MET_MAX_GROUPINGS distinct groupings.

    values: {(prefix + name, ((target, value bytes), ...) in the item's label order): float}, what CounterVec.With(labels).Add
    has summed. Regular expressions run on Python's `re`, which stands in for Go's RE2 (see the module's docstring)."""

    def __init__(self, items, prefix: str = ""):
        self.prefix, self.items, self.values = prefix, [], {}
        self.groupings = []
        for it in items:
            name = it.get("name", "")
            if it.get("type") != "counter":
                raise ValueError("metric %r: type %r is not counter" % (name, it.get("type")))
            if it.get("flatten"):
                raise ValueError("metric %r: flatten stays on the host path" % name)
            value_key = it.get("valueKey") or ""
            if value_key not in VALUE_FIELDS:
                raise ValueError("metric %r: value key %r is none of '', Bytes, Packets" % (name, value_key))
            remap = it.get("remap") or {}
            labels = [(l, remap.get(l) or l) for l in it.get("labels") or []]             # Preprocess: Remap[l] != "" renames
            filters = {}
            for f in it.get("filters") or []:
                filters.setdefault(f["key"], []).append(_Filter(f))
            dims = 0
            for key in [l for l, _ in labels] + [k for fs in filters.values() for f in fs for k in f.keys()]:
                if key not in KEY_DIMS:
                    raise ValueError("metric %r: key %r is outside the dimension list" % (name, key))
                dims |= KEY_DIMS[key]
            if dims not in self.groupings:
                self.groupings.append(dims)
            self.items.append(dict(name=prefix + name, grouping=self.groupings.index(dims), labels=labels, filters=filters, value_key=value_key,
                                   scale=float(it.get("valueScale") or 0)))
        if len(self.groupings) > L.MET_MAX_GROUPINGS:
            raise ValueError("%d distinct groupings, more than %d" % (len(self.groupings), L.MET_MAX_GROUPINGS))
        self.caps = [4096] * len(self.groupings)
        self._met = None

    def add_groups(self, groups, entries, labels, class_row) -> None:
        """prepareMetric + ProcessCounter per group: groups[g] is grouping g's METRIC_GROUP array. Two groups can land in one
        series (their keys differ, their label texts do not: a missing key and an empty value both print ""), so a series'
        integer sums are added up first and each series gets one Add of float(sum) / valueScale per call."""
        totals = {}
        for g, dims in enumerate(self.groupings):
            mine = [(k, it) for k, it in enumerate(self.items) if it["grouping"] == g]
            for group in groups[g]:
                m = group_keys(dims, group, entries, labels, class_row, g)
                for k, it in mine:
                    # ApplyFilters: the filters of one key are ORed, the keys ANDed
                    if not all(any(f(m) for f in fs) for fs in it["filters"].values()):
                        continue
                    total, series = VALUE_FIELDS[it["value_key"]]
                    if int(group[series]) == 0:                          # extractGenericValue: no flow of the group carries the key
                        continue
                    key = (k, tuple((target, convert_to_string(m[src]) if src in m else b"") for src, target in it["labels"]))
                    totals[key] = totals.get(key, 0) + int(group[total])
        for (k, series_labels), total in totals.items():
            it = self.items[k]
            value = float(total)
            if it["scale"] != 0:
                value /= it["scale"]
            key = (it["name"], series_labels)
            self.values[key] = self.values.get(key, 0.0) + value

    def observe(self, table, records, k8s, net=None, agent_ip=None) -> None:
        """The two resolves and the fold for these records on `table`'s device, then add_groups. k8s: the K8sTable (of `table`),
        net: the NetTable, required when a grouping selects a label or the direction. A cap that proves too small is grown and
        the fold repeated once."""
        if not self.items:
            return
        if net is None and any(d & NET_DIMS for d in self.groupings):
            raise ValueError("a grouping selects a subnet label or the direction: observe needs the net table")
        if self._met is None or self._met.k8s is not k8s or self._met._t is None:
            self._met = table.metrics_table(k8s, self.groupings)
        met = self._met
        k8s_rows = table.k8s_resolve(k8s, records)
        net_rows = table.net_resolve(net, records, k8s, k8s_rows, agent_ip) if net is not None else None
        rc, groups, counts = table.metrics_fold(met, records, k8s_rows, net_rows, self.caps)
        if rc == L.TRUNCATED:
            # a grouping that did not fit reports a lower bound only: the one retry takes the largest cap, and the next call a
            # cap sized by what the retry found
            over = [c > cap for c, cap in zip(counts, self.caps)]
            rc, groups, counts = table.metrics_fold(met, records, k8s_rows, net_rows, [L.MET_MAX_GROUPS if o else cap for o, cap in zip(over, self.caps)])
            if rc != L.OK:
                raise RuntimeError("more than %d groups in one grouping: %r" % (L.MET_MAX_GROUPS, counts))
            self.caps = [min(L.MET_MAX_GROUPS, max(cap, 1 << (2 * c).bit_length())) if o else cap for o, c, cap in zip(over, counts, self.caps)]
        self.add_groups(groups, k8s.entries, net.labels if net is not None else [], met.class_row)


CONTENT_KEY_DIMS = dict(DnsFlagsResponseCode=L.XDIM_DNS_RCODE, PktDropLatestDropCause=L.XDIM_DROP_CAUSE, PktDropLatestState=L.XDIM_DROP_STATE,
                        IPSecStatus=L.XDIM_IPSEC_STATUS)
VALUE_SOURCES = {"": L.MET_VALUE_NONE, "Bytes": L.MET_VALUE_BYTES, "Packets": L.MET_VALUE_PACKETS, "TimeFlowRttNs": L.MET_VALUE_RTT_NS,
                 "DnsLatencyMs": L.MET_VALUE_DNS_LATENCY_MS, "PktDropBytes": L.MET_VALUE_DROP_BYTES, "PktDropPackets": L.MET_VALUE_DROP_PACKETS}
DEF_BUCKETS = (.005, .01, .025, .05, .1, .25, .5, 1.0, 2.5, 5.0, 10.0)            # prometheus.DefBuckets
I64_MIN, I64_MAX = -2**63, 2**63 - 1
# the integers RecordToMap can write for a source (decode_protobuf.go:87-93,130-182, record.go:116-125): thresholds are searched here
SOURCE_DOMAIN = {L.MET_VALUE_RTT_NS: (I64_MIN, I64_MAX), L.MET_VALUE_DNS_LATENCY_MS: (-(2**63 // 10**6), (2**63 - 1) // 10**6),
                 L.MET_VALUE_DROP_BYTES: (0, 0xFFFF), L.MET_VALUE_DROP_PACKETS: (0, 0xFFFF), L.MET_VALUE_BYTES: (0, 2**64 - 1),
                 L.MET_VALUE_PACKETS: (0, 2**32 - 1)}
SIGNED_SOURCES = (L.MET_VALUE_RTT_NS, L.MET_VALUE_DNS_LATENCY_MS)


def scaled(x: int, scale: float) -> float:
    """What the histogram loop observes for the integer x: ConvertToFloat64, then / ValueScale unless that is 0."""
    v = float(x)
    return v / scale if scale != 0 else v


def threshold(bound: float, scale: float, lo: int, hi: int):
    """The largest integer x of [lo, hi] with scaled(x) <= bound, None if there is none: scaled does not decrease with x (scale
    >= 0), so `value <= threshold` on integers is `scaled(value) <= bound` on floats for every value of the domain."""
    if not scaled(lo, scale) <= bound:
        return None
    if scaled(hi, scale) <= bound:
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if scaled(mid, scale) <= bound:
            lo = mid
        else:
            hi = mid
    return lo


def content_keys(xdims: int, group, m: dict) -> dict:
    """The extra dimensions of one nfagg_metric_group_content into the map of group_keys, as RecordToMap writes them."""
    if xdims & L.XDIM_DNS_RCODE and int(group["dns_rcode"]) != 0xFF:
        m["DnsFlagsResponseCode"] = flp_enum_name(L.FLP_ENUM_DNS_RCODE, int(group["dns_rcode"]))
        m["DnsId"] = b"set"                                              # presence only: the id itself is no dimension
    if xdims & L.XDIM_DROP_CAUSE and int(group["drop_cause"]) != 0:
        m["PktDropLatestDropCause"] = flp_enum_name(L.FLP_ENUM_DROP_CAUSE, int(group["drop_cause"]))
    if xdims & L.XDIM_DROP_STATE and int(group["drop_state"]) != 0xFFFF:
        m["PktDropLatestState"] = flp_enum_name(L.FLP_ENUM_TCP_STATE, int(group["drop_state"]))
    if xdims & L.XDIM_IPSEC_STATUS and int(group["ipsec_status"]):
        m["IPSecStatus"] = b"error" if int(group["ipsec_status"]) == 2 else b"success"
    return m


class PromMetrics:
    """`encode prom` counters and histograms fed by nfagg_metrics_fold_content. items as PromCounters takes them, with type
    counter or histogram, the value keys "", Bytes, Packets, TimeFlowRttNs, DnsLatencyMs, PktDropBytes, PktDropPackets, and label
    and filter keys of KEY_DIMS and CONTENT_KEY_DIMS. A presence or absence filter on the item's own value key or on DnsId is
    served too: a flow without the value is skipped anyway, so presence of the own key filters nothing and absence alone leaves no
    series; DnsId exists exactly when the response code does. A grouping is (dims, xdims, bucketed source and thresholds) with up
    to two value slots; items share one where they can. ValueError for anything else, and for more than L.MET_MAX_GROUPINGS
    groupings, more than L.MET_MAX_BOUNDS buckets, buckets that do not increase, a negative valueScale, a Bytes bound whose
    threshold passes INT64_MAX.

    values: as PromCounters. histograms: {(prefix + name, labels): {"buckets": [count per bound, not cumulative, +Inf last],
    "count": int, "sum": float}}; per call and series the integer sum of the values is added up first and float(sum) / valueScale
    added once, the rule of the counters."""

    def __init__(self, items, prefix: str = "", item_buckets: bool = False):
        self.prefix, self.items, self.values, self.histograms = prefix, [], {}, {}
        self.groupings = []                      # dicts: dims, xdims, values (sources of the slots), hist (None or (source, thresholds))
        for it in items:
            name, kind = it.get("name", ""), it.get("type")
            if kind not in ("counter", "histogram"):
                raise ValueError("metric %r: type %r is neither counter nor histogram" % (name, kind))
            if it.get("flatten"):
                raise ValueError("metric %r: flatten stays on the host path" % name)
            value_key = it.get("valueKey") or ""
            if value_key not in VALUE_SOURCES:
                raise ValueError("metric %r: value key %r is none of %s" % (name, value_key, ", ".join(repr(k) for k in VALUE_SOURCES)))
            source = VALUE_SOURCES[value_key]
            scale = float(it.get("valueScale") or 0)
            if scale < 0:
                raise ValueError("metric %r: a negative valueScale" % name)
            remap = it.get("remap") or {}
            labels = [(l, remap.get(l) or l) for l in it.get("labels") or []]
            filters, dead = {}, False
            for f in it.get("filters") or []:
                filters.setdefault(f["key"], []).append(_Filter(f))
            dims = xdims = 0
            for key in list(filters):
                if key not in (value_key or None, "DnsId"):
                    continue
                if any(f.type not in ("presence", "absence") for f in filters[key]):
                    raise ValueError("metric %r: key %r serves presence and absence filters only" % (name, key))
                if key == value_key:             # ORed over the flows that have the value: presence is true, absence false
                    dead = dead or not any(f.type == "presence" for f in filters[key])
                    del filters[key]
                else:
                    xdims |= L.XDIM_DNS_RCODE
            for key in [l for l, _ in labels] + [k for fs in filters.values() for f in fs for k in f.keys()]:
                if key in KEY_DIMS:
                    dims |= KEY_DIMS[key]
                elif key in CONTENT_KEY_DIMS:
                    xdims |= CONTENT_KEY_DIMS[key]
                elif not (key == "DnsId" and key in filters):
                    raise ValueError("metric %r: key %r is outside the dimension lists" % (name, key))
            hist, bounds, skip = None, (), 0
            if kind == "histogram":
                if source == L.MET_VALUE_NONE:
                    raise ValueError("metric %r: a histogram needs a value key" % name)
                bounds = tuple(float(b) for b in it.get("buckets") or ()) if item_buckets and it.get("buckets") else DEF_BUCKETS
                if any(not a < b for a, b in zip(bounds, bounds[1:])):
                    raise ValueError("metric %r: buckets must increase" % name)
                lo, hi = SOURCE_DOMAIN[source]
                th = [threshold(b, scale, lo, hi) for b in bounds]
                skip = sum(1 for t in th if t is None)                   # bounds below the domain take no flow: dropped here, kept in the result
                dev = th[skip:]
                if not dev:
                    if lo == I64_MIN:
                        raise ValueError("metric %r: every bucket lies below the value's domain" % name)
                    dev, skip = [I64_MIN], len(bounds) - 1               # no value is <= INT64_MIN: everything goes to +Inf
                if any(t > I64_MAX for t in dev):
                    raise ValueError("metric %r: a bucket's threshold passes INT64_MAX" % name)
                if len(dev) > L.MET_MAX_BOUNDS:
                    raise ValueError("metric %r: %d buckets, more than %d" % (name, len(dev), L.MET_MAX_BOUNDS))
                hist = (source, tuple(dev))
            # a counter over Bytes, Packets or the flows reads the five sums every group has; the rest needs a value slot
            needs_slot = kind == "histogram" or source not in (L.MET_VALUE_NONE, L.MET_VALUE_BYTES, L.MET_VALUE_PACKETS)
            g = self._grouping(dims, xdims, source if needs_slot else None, hist)
            self.items.append(dict(name=prefix + name, kind=kind, grouping=g, labels=labels, filters=filters, value_key=value_key, source=source,
                                   slot=self.groupings[g]["values"].index(source) if needs_slot else None, scale=scale, dead=dead, bounds=bounds,
                                   skip=skip, n_dev=len(hist[1]) if hist else 0))
        if len(self.groupings) > L.MET_MAX_GROUPINGS:
            raise ValueError("%d distinct groupings, more than %d" % (len(self.groupings), L.MET_MAX_GROUPINGS))
        self.caps = [4096] * len(self.groupings)
        self._met = None

    def _grouping(self, dims, xdims, source, hist) -> int:
        for g, gr in enumerate(self.groupings):
            if (gr["dims"], gr["xdims"]) != (dims, xdims) or (hist is not None and gr["hist"] not in (None, hist)):
                continue
            if source is not None and source not in gr["values"] and len(gr["values"]) == 2:
                continue
            if source is not None and source not in gr["values"]:
                gr["values"].append(source)
            gr["hist"] = gr["hist"] or hist
            return g
        self.groupings.append(dict(dims=dims, xdims=xdims, values=[source] if source is not None else [], hist=hist))
        return len(self.groupings) - 1

    def specs(self):
        """The groupings as MetricsTable.spec takes them."""
        return [dict(dims=gr["dims"], xdims=gr["xdims"], value=tuple(gr["values"]), hist=gr["values"].index(gr["hist"][0]) + 1 if gr["hist"] else 0,
                     bounds=gr["hist"][1] if gr["hist"] else ()) for gr in self.groupings]

    @staticmethod
    def _value(it, group):
        """(integer sum of the item's value over the group's flows that have it, their number)."""
        if it["slot"] is None:
            total, series = VALUE_FIELDS[it["value_key"]]
            return int(group[total]), int(group[series])
        total = int(group["value_sum"][it["slot"]])
        if it["source"] in SIGNED_SOURCES and total >= 2**63:
            total -= 2**64
        return total, int(group["flows_with_value"][it["slot"]])

    def add_groups(self, groups, entries, labels, class_row) -> None:
        """prepareMetric + ProcessCounter / ProcessHist per group: groups[g] is grouping g's METRIC_GROUP_CONTENT array. As in
        PromCounters a series' integer sums are added up first; a histogram's buckets and count are integers throughout."""
        totals, hists = {}, {}
        for g, gr in enumerate(self.groupings):
            mine = [(k, it) for k, it in enumerate(self.items) if it["grouping"] == g and not it["dead"]]
            for group in groups[g]:
                m = content_keys(gr["xdims"], group, group_keys(gr["dims"], group, entries, labels, class_row, g))
                for k, it in mine:
                    if not all(any(f(m) for f in fs) for fs in it["filters"].values()):
                        continue
                    total, count = self._value(it, group)
                    if count == 0:                                       # extractGenericValue: no flow of the group carries the key
                        continue
                    key = (k, tuple((target, convert_to_string(m[src]) if src in m else b"") for src, target in it["labels"]))
                    if it["kind"] == "counter":
                        totals[key] = totals.get(key, 0) + total
                        continue
                    b = int(group["bucket"])
                    if b == L.MET_NO_BUCKET:
                        continue
                    h = hists.setdefault(key, [[0] * (len(it["bounds"]) + 1), 0, 0])
                    h[0][len(it["bounds"]) if b == it["n_dev"] else it["skip"] + b] += count
                    h[1] += count
                    h[2] += total
        for (k, series_labels), total in totals.items():
            it = self.items[k]
            key = (it["name"], series_labels)
            self.values[key] = self.values.get(key, 0.0) + scaled(total, it["scale"])
        for (k, series_labels), (buckets, count, total) in hists.items():
            it = self.items[k]
            h = self.histograms.setdefault((it["name"], series_labels), dict(buckets=[0] * len(buckets), count=0, sum=0.0))
            h["buckets"] = [a + b for a, b in zip(h["buckets"], buckets)]
            h["count"] += count
            h["sum"] += scaled(total, it["scale"])

    def observe(self, table, records, k8s, net=None, agent_ip=None, features=None) -> None:
        """The two resolves and the content fold for these records on `table`'s device, then add_groups. features: (present,
        parts) as FlowTable.map_merge returns and encode_flp_json_content takes them (or one dict with the present bytes under
        "present"); None: no flow has a part. A cap that proves too small is grown and the fold repeated once."""
        if not self.items:
            return
        if net is None and any(gr["dims"] & NET_DIMS for gr in self.groupings):
            raise ValueError("a grouping selects a subnet label or the direction: observe needs the net table")
        if isinstance(features, dict):
            features = (features.get("present"), {k: v for k, v in features.items() if k != "present"})
        if self._met is None or self._met.k8s is not k8s or self._met._t is None:
            self._met = table.metrics_table_specs(k8s, self.specs())
        met = self._met
        k8s_rows = table.k8s_resolve(k8s, records)
        net_rows = table.net_resolve(net, records, k8s, k8s_rows, agent_ip) if net is not None else None
        rc, groups, counts = table.metrics_fold_content(met, records, k8s_rows, net_rows, self.caps, features)
        if rc == L.TRUNCATED:
            over = [c > cap for c, cap in zip(counts, self.caps)]
            rc, groups, counts = table.metrics_fold_content(met, records, k8s_rows, net_rows,
                                                            [L.MET_MAX_GROUPS if o else cap for o, cap in zip(over, self.caps)], features)
            if rc != L.OK:
                raise RuntimeError("more than %d groups in one grouping: %r" % (L.MET_MAX_GROUPS, counts))
            self.caps = [min(L.MET_MAX_GROUPS, max(cap, 1 << (2 * c).bit_length())) if o else cap for o, c, cap in zip(over, counts, self.caps)]
        self.add_groups(groups, k8s.entries, net.labels if net is not None else [], met.class_row)
