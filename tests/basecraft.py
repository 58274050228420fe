"""Accounter-mode flows built from SCRIPTS (a helper module, no fixtures; numpy only), on tests/dedupcraft.py's Family, keys and
layouts. A script is the ordered list of records of ONE flow. model.AccumulateBase (pkg/model/flow_content.go:28-61) behind
"the first record is stored whole" (pkg/flow/account.go:95) reads ten fields, each by a rule of its own — least non-zero start,
greatest end, wrapping sums, or-ed flags, last non-zero eth_protocol / dscp / sampling, first non-zero MACs — so the orders of
values that tell one rule from its neighbours are enumerated outright: an exhaustive family holds EVERY sequence over its symbols,
of every length from 1 to its maximum.

    times   (start in {0, A, B}) x (end in {0, A, B}), A = 2^32 + 5, B = 7: nine symbols, lengths 1..4 — both 32-bit halves of
            either word move, independently and backwards; zero is "not set" for start and the least value for end
    lastnz  (dscp in {0, 40 + t, 0xFF - t}) x (sampling in {0, 1 + t, 0xFFFFFFFF - t}), eth_protocol following (d + s) mod 3 over
            {0, 0x0800 + t, 0xFFFF - t}: nine symbols, lengths 1..4 — all-ones values directly under the sequence tags
    macs    (src shape) x (dst shape) over SHAPES: 25 symbols, lengths 1..3 — MACs whose low 32 bits or high 16 bits are zero;
            sampling and dscp stay zero, so whether a record needs its sixth unit is decided by the MAC alone
    sums    (bytes in {0, 1, 2^63, 2^64 - 1}) x (packets in {0, 1, 2^31, 2^32 - 1}), flags = 1 << ((3 pos + symbol) mod 16):
            sixteen symbols, lengths 1..3 — the sums wrap, they do not saturate

t is the record's position in its script (mod STAMP, which only the seeded families reach): every non-zero value of lastnz and
macs carries it, so no two records of an exhaustive script agree in a non-zero field and "the first", "the last" and "the
largest" can be told apart. Whatever is not a family's subject stays as dedupcraft._blank leaves it, except the identity fields,
which carry the position in every family — if_index_first_seen = 1 + pos, direction_first_seen = pos & 1, ssl_version =
0x0300 + pos — so that "the first record is stored whole" shows everywhere.

Two seeded families draw from the union of the four symbol tables (59 symbols):

    wave    64 scripts of exactly 64 records: flow-major, one wave of 64 lanes holds a whole flow
    hot     8 scripts of 4 096 records: one cache entry folds thousands of records whose start and end are not monotone

start = 2^64 - 1 is in no family: the slots keep ~start and read it as "not set" (include/nfagg.h, nfagg_ingest)."""
import itertools
import zlib

import numpy as np

from dedupcraft import END_A, END_B, MAX_RECORDS, Family, _blank, _keys, flow_major, round_major, shuffled  # noqa: F401 (the layouts are re-exported)

EXHAUSTIVE = ("times", "lastnz", "macs", "sums")
SEEDED = ("wave", "hot")
FAMILIES = EXHAUSTIVE + SEEDED
MAX_LEN = {"times": 4, "lastnz": 4, "macs": 3, "sums": 3}
N_SYMBOLS = {"times": 9, "lastnz": 9, "macs": 25, "sums": 16}
WAVE_SCRIPTS, WAVE_LEN, HOT_SCRIPTS, HOT_LEN = 64, 64, 8, 4096
STAMP = 64                                                              # positions are stamped mod 64 (dscp is a byte)
DIGITS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"

TIMES = (0, END_A, END_B)
BYTES = (0, 1, 1 << 63, (1 << 64) - 1)
PACKETS = (0, 1, 1 << 31, (1 << 32) - 1)
# (the six bytes, the index of the last non-zero byte, +1 / -1: which way that byte moves with the stamp)
SHAPES = (((0, 0, 0, 0, 0, 0), 0, 0), ((0x02, 0, 0, 0, 0, 0), 0, 1), ((0, 0, 0x5e, 0, 0x01, 0x07), 5, 1), ((0, 0, 0, 0, 0, 0x09), 5, 1),
          ((0xff,) * 6, 5, -1))
DST_OFFSET = 64                                                         # dst carries the stamp t + 64: never src's byte


def _u(values, index, dtype=np.uint64):
    return np.array(values, dtype=dtype)[index]


def _macs(shape, stamp):
    """(n, 6) bytes: SHAPES[shape] with its last non-zero byte moved by the stamp."""
    out = np.array([s[0] for s in SHAPES], dtype=np.uint8)[shape]
    at, way = _u([s[1] for s in SHAPES], shape, np.int64), _u([s[2] for s in SHAPES], shape, np.int64)
    rows = np.arange(len(shape))
    out[rows, at] = (out[rows, at].astype(np.int64) + way * stamp).astype(np.uint8)
    return out


def _set_times(m, k, pos):
    m["start"], m["end"] = _u(TIMES, k // 3), _u(TIMES, k % 3)


def _set_lastnz(m, k, pos):
    t = (pos % STAMP).astype(np.uint64)
    d, s = k // 3, k % 3
    zero = np.zeros(len(k), dtype=np.uint64)
    m["dscp"] = np.choose(d, [zero, 40 + t, 0xFF - t])
    m["sampling"] = np.choose(s, [zero, 1 + t, 0xFFFFFFFF - t])
    m["eth_protocol"] = np.choose((d + s) % 3, [zero, 0x0800 + t, 0xFFFF - t])


def _set_macs(m, k, pos):
    t = pos % STAMP
    m["src_mac"], m["dst_mac"] = _macs(k // 5, t), _macs(k % 5, t + DST_OFFSET)


def _set_sums(m, k, pos):
    m["bytes"], m["packets"] = _u(BYTES, k // 4), _u(PACKETS, k % 4)
    m["flags"] = np.uint64(1) << ((3 * pos + k) % 16).astype(np.uint64)


SETTERS = {"times": _set_times, "lastnz": _set_lastnz, "macs": _set_macs, "sums": _set_sums}
UNION = [(name, k) for name in EXHAUSTIVE for k in range(N_SYMBOLS[name])]       # symbol number of a seeded family -> (table, symbol)
_UNION_START = {name: UNION.index((name, 0)) for name in EXHAUSTIVE}


def _apply(tables, recs, sym, pos):
    """Write symbol sym[i] at position pos[i] into record i. tables: the one table of an exhaustive family, or all four (sym then
    numbers the union)."""
    m = recs["metrics"]
    for name in tables:
        lo = _UNION_START[name] if len(tables) > 1 else 0
        at = np.nonzero((sym >= lo) & (sym < lo + N_SYMBOLS[name]))[0]
        if len(at):
            part = m[at]
            SETTERS[name](part, sym[at] - lo, pos[at])
            m[at] = part


class BaseFamily(Family):
    """dedupcraft.Family whose symbols depend on the position: `tables` names the symbol tables the records are built from."""

    def __init__(self, name, tables, recs, script, pos, keys):
        Family.__init__(self, name, recs, script, pos, keys, symbols=None)
        self.tables = tables
        self.n_symbols = sum(N_SYMBOLS[t] for t in tables)

    def symbol_numbers(self):
        """The symbol of every record re-derived from the RECORDS: the one symbol whose record at that position has these bytes."""
        want = self.recs.view(np.uint8).reshape(-1, 144)
        out, hits = np.full(len(self.recs), -1, dtype=np.int64), np.zeros(len(self.recs), dtype=np.int64)
        for k in range(self.n_symbols):
            trial = _plain(self.script, self.pos, self.keys)
            _apply(self.tables, trial, np.full(len(trial), k, dtype=np.int64), self.pos)
            ok = (trial.view(np.uint8).reshape(-1, 144) == want).all(axis=1)
            out[ok] = k
            hits += ok
        assert (hits == 1).all(), "a record matches no symbol, or several"
        return out

    def describe(self, s):
        if getattr(self, "_sym", None) is None:
            self._sym = self.symbol_numbers()
        text = "".join(DIGITS[k] for k in self._sym[self.start[s]:self.start[s] + min(int(self.length[s]), 80)])
        return "%s script %d = '%s%s'" % (self.name, s, text, "..." if self.length[s] > 80 else "")


def _plain(script, pos, keys):
    """dedupcraft's blank record with the position in the identity fields."""
    recs = _blank(script, pos, keys)
    m = recs["metrics"]
    m["if_index_first_seen"], m["direction_first_seen"], m["ssl_version"] = 1 + pos, pos & 1, 0x0300 + pos
    return recs


def _build(name, tables, seqs):
    """seqs: one array (n_k, k) of symbol numbers per length."""
    script = np.concatenate([np.repeat(np.arange(len(q)), q.shape[1]) + off
                             for q, off in zip(seqs, np.cumsum([0] + [len(q) for q in seqs[:-1]]))])
    pos = np.concatenate([np.tile(np.arange(q.shape[1]), len(q)) for q in seqs])
    sym = np.concatenate([q.reshape(-1) for q in seqs])
    keys = _keys("base " + name, sum(len(q) for q in seqs))
    recs = _plain(script, pos, keys)
    _apply(tables, recs, sym, pos)
    return BaseFamily(name, tables, recs, script, pos, keys)


def exhaustive(name):
    n = N_SYMBOLS[name]
    return _build(name, (name,), [np.array(list(itertools.product(range(n), repeat=k)), dtype=np.int64) for k in range(1, MAX_LEN[name] + 1)])


def seeded(name):
    n_scripts, length = {"wave": (WAVE_SCRIPTS, WAVE_LEN), "hot": (HOT_SCRIPTS, HOT_LEN)}[name]
    rng = np.random.default_rng(zlib.crc32(("basecraft %s symbols" % name).encode()))
    return _build(name, EXHAUSTIVE, [rng.integers(0, len(UNION), size=(n_scripts, length))])


_cache = {}


def family(name):
    """The family of that name, built once per process. Treat its arrays as read-only."""
    if name not in _cache:
        _cache[name] = exhaustive(name) if name in EXHAUSTIVE else seeded(name)
    return _cache[name]


def digest(fam):
    """crc32 of the family's records (tests/golden/basecraft_digest.json pins it: a changed builder does not pass unnoticed)."""
    return zlib.crc32(np.ascontiguousarray(fam.recs).view(np.uint8).tobytes())
