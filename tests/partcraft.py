"""Per-CPU partials built from SCRIPTS (a helper module, no fixtures; numpy only). A script is the ordered list of the per-CPU
partials of ONE flow in one feature map — n_cpu is the script's length — and the six folds of pkg/model/flow_content.go:63-198
(AccumulateDNS, Drops, NetworkEvents, Xlat, Additional, Quic behind buildBaseFromAdditional) each read a handful of small fields:
the orders of values that matter are enumerated, every sequence over a family's symbols of every length from 1 to 3.

    additional  ipsec_encrypted_ret in {-2^31, 0, 2^31 - 1} x ipsec_encrypted in {0, 1} x flow_rtt in {0, 5, 2^63}: 18 symbols —
                the signed compare, the three-way rule of ret, an unsigned 64-bit maximum
    dns         id in {0, 7 + pos, 0xFFFF - pos} x errno in {0, 5 + pos} x latency in {0, 9, 2^63}; flags one-hot by position,
                name = the position: 18 symbols — a later CPU with errno 0 resets errno and nothing else, the name stays CPU 0's
    drops       bytes in {0, 1, 0x8000, 0xFFFF}, packets the same list reversed, x (cause, state) in {00, c0, 0s, cs}: 16 symbols —
                0x8000 + 0x8000, 0xFFFF + 0, 0xFFFF + 1, 1 + 0xFFFF
    quic        version in {0, 1, 2^31, 2^32 - 1} x seen in {0, 1, 255} (long = the class, short = reversed): 12 symbols
    xlat        saddr form x daddr form over FORMS (::, ::ffff:0.0.0.0, ::ffff:0.0.0.1, the near-miss with bytes 10, 11 = 00, ff,
                2001:db8::1); ports and zone carry the position: 25 symbols
    netev       one event per partial: slot in {0, 3} x metadata in {all-zero, a, b} x packets in {0, 1, 0xFFFF}, bytes alongside;
                CPU 0's network_events_idx = script mod 4: 18 symbols
    ring        (seeded) 2 000 scripts of 8 CPUs, one or two events per partial from a pool of six metadata values plus all-zero
    walk        every subset of the six feature maps, with and without a main-map row (128 flows), at n_cpu 1 and 2: each map's
                partial has its own eth_protocol, start and end, so the merged base tells which map buildBaseFromAdditional saw
                first — tracer.go:1057-1110 walks dns, drops, network events, xlat, additional, quic

In every family a partial's start / end cycle over the nine (start, end) pairs of {0, A, B}^2 (A = 2^32 + 5, B = 7), its
eth_protocol over {0, 0x0800 + pos}, and the caller's base metrics over {zeroes, start = end = A, start = end = B}. Every length-3
script also runs EMBEDDED: its partials at CPUs (0, k, n_cpu - 1) of an otherwise all-zero slice, n_cpu in 5..9, k = 1 + script
mod (n_cpu - 2) — the zero CPUs are folded too (an all-zero DNS partial resets errno), and a four-way unrolled loop sees every
tail length."""
import itertools
import zlib

import numpy as np

from dedupcraft import END_A, END_B, _keys
from oracle.oracle import ADDITIONAL, DNS, DROPS, FLOW_ID, FLOW_METRICS, NETEV, QUIC, XLAT

EXHAUSTIVE = ("additional", "dns", "drops", "quic", "xlat", "netev")
FAMILIES = EXHAUSTIVE + ("ring",)
KIND = {"additional": "additional", "dns": "dns", "drops": "drops", "quic": "quic", "xlat": "xlat", "netev": "network_events", "ring": "network_events"}
DTYPE = {"additional": ADDITIONAL, "dns": DNS, "drops": DROPS, "network_events": NETEV, "xlat": XLAT, "quic": QUIC}
N_SYMBOLS = {"additional": 18, "dns": 18, "drops": 16, "quic": 12, "xlat": 25, "netev": 18}
MAX_LEN = 3
EMBED_CPUS = (5, 6, 7, 8, 9)
RING_SCRIPTS, RING_CPUS = 2000, 8
WALK = ("dns", "drops", "network_events", "xlat", "additional", "quic")               # tracer.go:1057-1110
ENUM = ("additional", "dns", "drops", "network_events", "xlat", "quic")               # NFAGG_ROLLUP_*

TIMES = (0, END_A, END_B)
RET, RTT = (-(1 << 31), 0, (1 << 31) - 1), (0, 5, 1 << 63)
LATENCY = (0, 9, 1 << 63)
DROP_COUNTS = (0, 1, 0x8000, 0xFFFF)
VERSIONS, SEEN = (0, 1, 1 << 31, (1 << 32) - 1), (0, 1, 255)
FORMS = np.array([[0] * 16, [0] * 10 + [0xff, 0xff, 0, 0, 0, 0], [0] * 10 + [0xff, 0xff, 0, 0, 0, 1], [0] * 10 + [0, 0xff, 0, 0, 0, 0],
                  [0x20, 0x01, 0x0d, 0xb8] + [0] * 11 + [1]], dtype=np.uint8)
MD = np.array([[0] * 8, [1, 2, 3, 4, 5, 6, 7, 8], [0, 0, 0, 0, 0, 0, 0, 9]], dtype=np.uint8)     # all-zero, a, b
EV_PACKETS, EV_BYTES = (0, 1, 0xFFFF), (0, 0x8000, 0xFFFF)
RING_POOL = np.array([[0] * 8] + [[k, 0, 0, 0, 0, 0, 0, k + 1] for k in range(1, 7)], dtype=np.uint8)


def _u(values, index, dtype=np.uint64):
    return np.array(values, dtype=dtype)[index]


def _common(p, script, pos):
    """start / end / eth_protocol of every partial, by script and position."""
    c = (script + 4 * pos) % 9
    p["start"], p["end"] = _u(TIMES, c // 3), _u(TIMES, c % 3)
    p["eth_protocol"] = np.where((script + pos) % 2 == 0, 0, 0x0800 + pos)


def _set_additional(p, k, pos, script):
    p["ipsec_ret"], p["ipsec_encrypted"], p["flow_rtt"] = _u(RET, k // 6, np.int64), (k // 3) % 2, _u(RTT, k % 3)


def _set_dns(p, k, pos, script):
    zero = np.zeros(len(k), dtype=np.int64)
    p["id"] = np.choose(k // 6, [zero, 7 + pos, 0xFFFF - pos])
    p["err_no"] = np.choose((k // 3) % 2, [zero, 5 + pos])
    p["latency"] = _u(LATENCY, k % 3)
    p["flags"] = 1 << pos
    p["name"] = (0x61 + pos)[:, None]


def _set_drops(p, k, pos, script):
    p["bytes"], p["packets"] = _u(DROP_COUNTS, k // 4), _u(DROP_COUNTS, 3 - k // 4)
    p["latest_drop_cause"] = np.where(k % 4 & 1, 100 + pos, 0)
    p["latest_state"] = np.where(k % 4 & 2, 10 + pos, 0)
    p["latest_flags"] = 1 << pos


def _set_quic(p, k, pos, script):
    p["version"] = _u(VERSIONS, k // 3)
    p["seen_long_hdr"], p["seen_short_hdr"] = _u(SEEN, k % 3), _u(SEEN, 2 - k % 3)


def _set_xlat(p, k, pos, script):
    p["saddr"], p["daddr"] = FORMS[k // 5], FORMS[k % 5]
    p["sport"], p["dport"], p["zone_id"] = 1000 + pos, 2000 + pos, 1 + pos


def _set_netev(p, k, pos, script):
    slot = np.where(k // 9 == 0, 0, 3)
    rows = np.arange(len(k))
    ev, by, pk = p["network_events"], p["bytes"], p["packets"]
    ev[rows, slot] = MD[(k // 3) % 3]
    pk[rows, slot], by[rows, slot] = _u(EV_PACKETS, k % 3), _u(EV_BYTES, k % 3)
    p["network_events"], p["bytes"], p["packets"] = ev, by, pk
    p["network_events_idx"] = np.where(pos == 0, script % 4, pos & 3)


SETTERS = {"additional": _set_additional, "dns": _set_dns, "drops": _set_drops, "quic": _set_quic, "xlat": _set_xlat, "netev": _set_netev}


def base_metrics(script):
    """The caller's base metrics of every script: zeroes, start = end = A (no eth_protocol), start = end = B (IPv6)."""
    b = np.zeros(len(script), dtype=FLOW_METRICS)
    cls = script % 3
    b["start"] = b["end"] = _u(TIMES, cls)
    b["eth_protocol"] = np.where(cls == 2, 0x86DD, 0)
    b["packets"], b["bytes"] = 1 + script % 7, 100 + script                  # what the folds must leave alone
    return b


class Call:
    """One rollup: `parts` (n_flows, n_cpu) of `kind`, the callers' `base` (n_flows), the script of every flow, and for an
    embedded call the CPUs (n_flows, 3) the script's partials sit at (None otherwise)."""

    def __init__(self, kind, parts, base, script, at=None):
        self.kind, self.parts, self.base, self.script, self.at = kind, parts, base, script, at
        self.n_cpu = parts.shape[1]


class PartFamily:
    def __init__(self, name, kind, seqs, calls, keys):
        self.name, self.kind, self.seqs, self.calls, self.keys = name, kind, seqs, calls, keys
        self.n_scripts = len(seqs)

    def describe(self, s):
        return "%s script %d = %s" % (self.name, s, "".join("0123456789abcdefghijklmnopqrstuvwxyz"[k] for k in self.seqs[s]) if self.seqs[s] is not None else "(seeded)")

    def ids(self, scripts):
        return np.ascontiguousarray(self.keys[scripts]).view(FLOW_ID).reshape(-1)


def exhaustive(name):
    kind, n = KIND[name], N_SYMBOLS[name]
    dt = DTYPE[kind]
    seqs, calls, first = [], [], 0
    for length in range(1, MAX_LEN + 1):
        q = np.array(list(itertools.product(range(n), repeat=length)), dtype=np.int64)
        script = first + np.arange(len(q))
        parts = np.zeros((len(q), length), dtype=dt)
        for pos in range(length):
            col = parts[:, pos].copy()
            _common(col, script, np.full(len(q), pos))
            SETTERS[name](col, q[:, pos], np.full(len(q), pos), script)
            parts[:, pos] = col
        calls.append(Call(kind, parts, base_metrics(script), script))
        seqs += [tuple(r) for r in q.tolist()]
        first += len(q)
    three = calls[-1]
    for n_cpu in EMBED_CPUS:
        at = np.stack([np.zeros(len(three.script), dtype=np.int64), 1 + three.script % (n_cpu - 2), np.full(len(three.script), n_cpu - 1)], axis=1)
        parts = np.zeros((len(three.script), n_cpu), dtype=dt)
        for pos in range(3):
            parts[np.arange(len(at)), at[:, pos]] = three.parts[:, pos]
        calls.append(Call(kind, parts, three.base, three.script, at))
    return PartFamily(name, kind, seqs, calls, _keys("part " + name, first))


def ring():
    """Seeded: per partial one or two events in slots 0 and 1, metadata from RING_POOL (row 0 is all-zero), packets and bytes from
    {0, 1, 0x7000, 0xFFFF} weighted towards non-zero; every partial's network_events_idx in 0..3 (CPU 0's is the one that counts)."""
    rng = np.random.default_rng(zlib.crc32(b"partcraft ring"))
    n, c = RING_SCRIPTS, RING_CPUS
    script = np.arange(n)
    parts = np.zeros((n, c), dtype=NETEV)
    for pos in range(c):
        col = parts[:, pos].copy()
        _common(col, script, np.full(n, pos))
        two = rng.random(n) < 0.5
        for slot in (0, 1):
            on = two | (slot == 0)
            col["network_events"][on, slot] = RING_POOL[rng.integers(0, len(RING_POOL), n)][on]
            col["packets"][on, slot] = rng.choice([0, 1, 0x7000, 0xFFFF, 0xFFFF], n)[on]
            col["bytes"][on, slot] = rng.choice([0, 1, 0x7000, 0xFFFF], n)[on]
        col["network_events_idx"] = rng.integers(0, 4, n)
        parts[:, pos] = col
    return PartFamily("ring", "network_events", [None] * n, [Call("network_events", parts, base_metrics(script), script)], _keys("part ring", n))


class Walk:
    """128 ids: id s has a main-map row when s & 64, and stands in feature map WALK[j] when s >> j & 1 (id 0 stands nowhere)."""

    def __init__(self, n_cpu):
        self.n_cpu = n_cpu
        self.keys = _keys("part walk", 128)
        s = np.arange(128)
        ids = np.ascontiguousarray(self.keys).view(FLOW_ID).reshape(-1)
        has_main = (s & 64) != 0
        self.main_ids = ids[has_main]
        self.main_vals = np.zeros(int(has_main.sum()), dtype=FLOW_METRICS)          # no eth_protocol, no times: the feature maps decide
        self.main_vals["packets"], self.main_vals["bytes"] = 3, 300
        self.feats = {}
        for j, kind in enumerate(WALK):
            rows = s[(s >> j & 1) != 0]
            v = np.zeros((len(rows), n_cpu), dtype=DTYPE[kind])
            for cpu in range(n_cpu):
                v["eth_protocol"][:, cpu] = 0x1000 * (cpu + 1) + ENUM.index(kind)    # its own eth_protocol, start and end
                v["start"][:, cpu] = 1000 - 100 * j + cpu
                v["end"][:, cpu] = 2000 + 100 * j + cpu
            self.feats[kind] = (ids[rows], v)
        self.n_flows = 127

    def first_map(self, s):
        """The first map of the walk that holds id s (None: none does)."""
        return next((kind for j, kind in enumerate(WALK) if s >> j & 1), None)


_cache = {}


def family(name):
    """The family of that name, built once per process. Treat its arrays as read-only."""
    if name not in _cache:
        _cache[name] = ring() if name == "ring" else exhaustive(name)
    return _cache[name]


def walk(n_cpu):
    if ("walk", n_cpu) not in _cache:
        _cache["walk", n_cpu] = Walk(n_cpu)
    return _cache["walk", n_cpu]


def merge_maps(fam, call):
    """The maps of one map merge over a call's flows: every script's partials in the family's feature map, and a main-map row (the
    call's base metrics) for the EVEN scripts only."""
    even = call.script % 2 == 0
    return fam.ids(call.script[even]), call.base[even], {fam.kind: (fam.ids(call.script), call.parts)}
