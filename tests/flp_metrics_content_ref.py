"""Independent restatement of flowlogs-pipeline's `encode prom` histograms, per flow, beside the counters of
tests/flp_metrics_ref.py (taken as they are), over the maps of tests/flp_json_content_ref.add_content +
tests/flp_json_net_ref.apply_rules: the MapTracer flow's DNS, drop, RTT and IPsec keys are in those maps exactly when
RecordToMap writes them. No import of the product; it knows nothing of groups, buckets as key dimensions or integer thresholds.
Paths under flowlogs-pipeline's pkg/:

  pipeline/encode/metrics_common.go:144-159       MetricCommonEncode's histogram loop: prepareMetric, ProcessHist
  pipeline/encode/metrics_common.go:179-211       prepareMetric: filters, extractGenericValue, ConvertToFloat64, / ValueScale
  pipeline/encode/encode_prom.go:78-86            ProcessHist: With(labels).Observe(value)
  pipeline/encode/encode_prom.go:130-134          addHistogram: HistogramOpts{Name, Help} WITHOUT Buckets, so prometheus.DefBuckets
                                                  whatever the item says (item_buckets=True restates newer FLP, which passes them)
  client_golang histogram.Observe                 sort.SearchFloat64s(upperBounds, v): the first bound >= v, else +Inf; count and
                                                  sum (a float addition per observation) per series

There is no Go toolchain here: this file is pinned by reading, and by the vectors of tests/test_export_reference_vectors.py for
the presence of the keys it reads."""
import bisect

import flp_metrics_ref as M

DEF_BUCKETS = [.005, .01, .025, .05, .1, .25, .5, 1, 2.5, 5, 10]           # prometheus.DefBuckets


class Histograms:
    """values[(prefix + name, labels)] = {"buckets": [observations per bound, not cumulative, +Inf last], "count", "sum"}, all
    three as running values: one Observe per flow."""

    def __init__(self, items, prefix: str = "", item_buckets: bool = False):
        self.pre = [M.preprocess(it) for it in items]
        self.bounds = [[float(b) for b in it["buckets"]] if item_buckets and it.get("buckets") else DEF_BUCKETS for it in items]
        self.prefix, self.values = prefix, {}

    def encode(self, flow: dict) -> None:
        for pre, bounds in zip(self.pre, self.bounds):                         # metrics_common.go:144-159
            if not M.apply_filters(flow, pre):
                continue
            val = M.extract_generic_value(flow, pre)
            if val is None:                                                    # skipped before its labels are registered
                continue
            v = float(val)                                                     # ConvertToFloat64
            if pre["scale"] != 0:
                v /= pre["scale"]
            key = (self.prefix + pre["name"], M.extract_labels(flow, pre))
            h = self.values.setdefault(key, dict(buckets=[0] * (len(bounds) + 1), count=0, sum=0.0))
            h["buckets"][bisect.bisect_left(bounds, v)] += 1                   # sort.SearchFloat64s
            h["count"] += 1
            h["sum"] += v


def exact_sums(maps, items, prefix: str = "") -> dict:
    """Per series the exact integer sum of the value over the flows the restatement's own filters and labels select."""
    out = {}
    for pre in (M.preprocess(it) for it in items):
        for m in maps:
            if M.apply_filters(m, pre) and M.extract_generic_value(m, pre) is not None:
                key = (prefix + pre["name"], M.extract_labels(m, pre))
                out[key] = out.get(key, 0) + int(M.extract_generic_value(m, pre))
    return out
