"""flowlogs-pipeline's `extract timebased` stage (pkg/pipeline/extract/extract_timebased.go, extract/timebased/*.go,
api/extract_timebased.go) over the GPU's windowed GROUP BY and top-K (nfagg_timebased_*): the host mirror that parses the
stage's rules, feeds a call's flows to the device and turns the few results back into the maps CreateGenericMap builds.

The reference keeps per table and key a list of (stamp, flow map) and walks all of it for every rule of every call; here the
device keeps one slice of per-key integer partials per call, and this module sees K results per rule.

Served index keys: SrcAddr, DstAddr, SrcPort, DstPort, Proto, SrcK8S_* / DstK8S_* (one field each), SrcSubnetLabel,
DstSubnetLabel, FlowDirection. Served operation keys: Bytes, Packets, TimeFlowRttNs, DnsLatencyMs, PktDropBytes, PktDropPackets.
Anything else raises ValueError: such a rule stays on the host path.

Not restated, by design: a flow that enters a table without the operation key of one of its rules makes the reference panic
(ConvertToFloat64 of a missing key); extract() raises MissingOperationKey and changes nothing, the caller filters those flows
out first (TransformFilter with a presence rule). Keys are capped per table (max_keys): TimebasedOverflow, then reset()."""
from . import _lib as L
from .conntrack import parse_duration
from .filter import go_ip_string
from .metrics import K8S_SUFFIXES, VALUE_SOURCES
from .table import K8S_FIELDS

OPERATIONS = {"sum": L.TB_OP_SUM, "avg": L.TB_OP_AVG, "min": L.TB_OP_MIN, "max": L.TB_OP_MAX, "count": L.TB_OP_COUNT, "last": L.TB_OP_LAST,
              "diff": L.TB_OP_DIFF}
PLAIN_KEYS = ("SrcAddr", "DstAddr", "SrcPort", "DstPort", "Proto", "SrcSubnetLabel", "DstSubnetLabel", "FlowDirection")
K8S_KEYS = {side + "K8S_" + s: (k, f) for k, side in enumerate(("Src", "Dst")) for f, s in enumerate(K8S_SUFFIXES)}
NET_KEYS = ("SrcSubnetLabel", "DstSubnetLabel", "FlowDirection")


class MissingOperationKey(RuntimeError):
    """Some flows enter a table but lack the operation key of one of its rules; `count` is their number. Nothing was changed."""

    def __init__(self, count: int):
        super().__init__("%d flows enter a table without the operation key of one of its rules" % count)
        self.count = count


class TimebasedOverflow(RuntimeError):
    """A table met more distinct keys than max_keys. The stage is unusable until reset()."""


def parse_rules(cfg):
    """CreateIndexKeysAndFilters (timebased.go:56-107) over cfg = {"rules": [...]} (or the list itself): returns (rules,
    skipped, tables). rules: the filters in order, dicts of name, index_key (the joined string), index_keys, operation, operation_key,
    top_k, reversed, interval_ns. skipped: [(rule, reason)] for a rule without index keys or with an illegal operation, as the
    reference logs and drops them. tables: {index_key: max interval_ns}, including the table of a rule dropped for its
    operation, which the reference has created by then."""
    items = (cfg.get("rules") or []) if isinstance(cfg, dict) else list(cfg)
    rules, skipped, tables = [], [], {}
    for it in items:
        keys = list(it.get("indexKeys") or [])
        if keys:
            index_key = ",".join(keys)
        elif it.get("indexKey"):
            index_key, keys = it["indexKey"], [it["indexKey"]]
        else:
            skipped.append((it, "missing IndexKey(s)"))
            continue
        interval = parse_duration(it.get("timeInterval") or 0)
        tables[index_key] = max(tables.get(index_key, interval), interval)
        op = it.get("operationType") or ""
        if op not in OPERATIONS:
            skipped.append((it, "illegal operation type %s" % op))
            continue
        rules.append(dict(name=it.get("name", ""), index_key=index_key, index_keys=keys, operation=op, operation_key=it.get("operationKey", ""),
                          top_k=int(it.get("topK") or 0), reversed=bool(it.get("reversed")), interval_ns=interval))
    return rules, skipped, tables


def render_column(key: str, col, tb, table: int, column: int) -> str:
    """One column of a nfagg_tb_key as the reference's ConvertToString prints the flow's value: net.IP.String() for an
    address, decimal for a port, the protocol and the direction, the Kubernetes entry's text for a class, the label's text."""
    raw = bytes(col)
    if key in ("SrcAddr", "DstAddr"):
        return go_ip_string(raw).decode()
    v = int.from_bytes(raw[:4], "little")
    if key in ("SrcPort", "DstPort", "Proto", "FlowDirection"):
        return "%d" % v
    if key in ("SrcSubnetLabel", "DstSubnetLabel"):
        text = tb.net.labels[v]
        return text.decode("utf-8", "surrogateescape") if isinstance(text, (bytes, bytearray)) else str(text)
    _, f = K8S_KEYS[key]
    text = tb.k8s.entries[tb.class_row(table, column, v)][1].get(K8S_FIELDS[f]) or b""
    return text.decode("utf-8", "surrogateescape") if isinstance(text, (bytes, bytearray)) else str(text)


class ExtractTimebased:
    """The stage on `table`'s device. rules: the stage's configuration ({"rules": [...]}, or the list), parsed by parse_rules;
    skipped rules are in `.skipped`. k8s / net: the K8sTable / NetTable of `table`, required when a rule names a Kubernetes key /
    a subnet label or the direction. max_keys: the cap on distinct keys per table.

    extract(records, now_unix_ns, features=None) is Extract(entries) at that time: it returns the list of maps, rule after
    rule: name, index_key, operation, <operationKey>: float, and every index key with its text. `inexact` holds, per returned
    map, whether the value carries NFAGG_TB_INEXACT."""

    def __init__(self, table, rules, k8s=None, net=None, max_keys: int = 1 << 16, agent_ip=None):
        self.table, self.k8s, self.net, self.agent_ip = table, k8s, net, agent_ip
        self.rules, self.skipped, self.tables = parse_rules(rules)
        specs = []
        for ru in self.rules:
            for key in ru["index_keys"]:
                if key not in PLAIN_KEYS and key not in K8S_KEYS:
                    raise ValueError("rule %r: index key %r is not served" % (ru["name"], key))
                if key in K8S_KEYS and k8s is None:
                    raise ValueError("rule %r: index key %r needs the Kubernetes table" % (ru["name"], key))
                if key in NET_KEYS and net is None:
                    raise ValueError("rule %r: index key %r needs the net table" % (ru["name"], key))
            if len(ru["index_keys"]) > L.TB_MAX_COLUMNS:
                raise ValueError("rule %r: %d index keys, more than %d" % (ru["name"], len(ru["index_keys"]), L.TB_MAX_COLUMNS))
            source = VALUE_SOURCES.get(ru["operation_key"], L.MET_VALUE_NONE)
            if source == L.MET_VALUE_NONE:
                raise ValueError("rule %r: operation key %r is none of %s" % (ru["name"], ru["operation_key"],
                                                                              ", ".join(repr(k) for k in VALUE_SOURCES if k)))
            if not 0 <= ru["top_k"] <= L.TB_MAX_TOPK:
                raise ValueError("rule %r: topK %d is outside 0..%d" % (ru["name"], ru["top_k"], L.TB_MAX_TOPK))
            specs.append(dict(index_keys=ru["index_keys"], operation=OPERATIONS[ru["operation"]], value=source, top_k=ru["top_k"],
                              reversed=ru["reversed"], interval_ns=ru["interval_ns"]))
        self.inexact = []
        self._tb = table.timebased_rules(specs, k8s, net, max_keys) if specs else None
        self._caps = [max(ru["top_k"], 64) for ru in self.rules]

    def close(self):
        if self._tb is not None:
            self._tb.close()
            self._tb = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        if self._tb is not None:
            self._tb.reset()

    def stats(self):
        return self._tb.stats() if self._tb is not None else None

    def maps(self, results):
        """CreateGenericMap (filters.go:167-191) of every rule's results."""
        out, self.inexact = [], []
        for r, (ru, res) in enumerate(zip(self.rules, results)):
            t = self._tb.table_of_rule[r]
            keys = self._tb.keys(t, res["key"]) if len(res) else []
            for k in range(len(res)):
                m = {"name": ru["name"], "index_key": ru["index_key"], "operation": ru["operation"], ru["operation_key"]: float(res["value"][k])}
                for c, key in enumerate(ru["index_keys"]):
                    m[key] = render_column(key, keys[k]["col"][c], self._tb, t, c)
                out.append(m)
                self.inexact.append(bool(int(res["flags"][k]) & L.TB_INEXACT))
        return out

    def extract(self, records, now_unix_ns: int, features=None):
        if self._tb is None:
            return []
        if isinstance(features, dict):
            features = (features.get("present"), {k: v for k, v in features.items() if k != "present"})
        need_k8s = any(k in K8S_KEYS for ru in self.rules for k in ru["index_keys"])
        need_net = any(k in NET_KEYS for ru in self.rules for k in ru["index_keys"])
        n = len(records)
        k8s_rows = self.table.k8s_resolve(self.k8s, records) if (need_k8s or (need_net and self.k8s is not None)) and n else None
        net_rows = self.table.net_resolve(self.net, records, self.k8s, k8s_rows, self.agent_ip) if need_net and n else None
        rc, results, counts, missing = self.table.timebased_extract(self._tb, records, now_unix_ns, k8s_rows if need_k8s else None, net_rows, features,
                                                                    self._caps)
        if rc == L.EDEFER:
            raise MissingOperationKey(missing)
        if rc == L.TRUNCATED:
            if self._tb.stats().failed:
                raise TimebasedOverflow("a table has met more than max_keys = %d distinct keys" % self._tb.max_keys)
            self._caps = [max(cap, 2 * c) for cap, c in zip(self._caps, counts)]      # the windows have advanced: only the results are taken again
            rc, results, counts = self.table.timebased_results(self._tb, self._caps)
            if rc != L.OK:
                raise RuntimeError("nfagg_timebased_results: %d" % rc)
        return self.maps(results)
