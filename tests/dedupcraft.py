"""Kernel-dedup flows built from SCRIPTS (a helper module, no fixtures; numpy only).

A script is the ordered list of records of ONE flow; a family is a set of scripts, one distinct flow key per script. The merge that
kernel-dedup mode restates (bpf/flows.c:76-143 update_existing_flow + add_observed_intf) reads a handful of small fields, so the
orders of events that matter are enumerated outright instead of being left to a seed: an exhaustive family holds EVERY sequence over
its symbol set, of every length from 1 to its maximum. Whatever is not a family's subject is fixed and plain: one packet and 100
bytes per record, `end` growing by one per record, TLS fields zero, an empty observed list on the first record.

    intf      (if_index_first_seen in {0, 1, 2}) x (direction_first_seen in {0, 1}): six symbols, lengths 1..5 — F = 0 flows, records
              on interface 0 that are ignored (their end and flags too), side before / after counted, the merge to BOTH
    ssl       (interface in {1, 2}) x (ssl_version in {0, 0x0303, 0x0304}): six symbols, lengths 1..5 — flows.c:111-118
    hello     (interface) x (tls_types in {1, 2}) x (tls_cipher_suite in {0, 0x1301, 0xc02f}, tls_key_share moving with it over
              {0, 0x001d, 0x0017}): twelve symbols, lengths 1..3 (length 4 alone would be 82 944 records) — flows.c:119-125
    last      (interface) x (class in {zero, a, b}): the class sets dscp, sampling and end together; end a = 2^32 + 5, b = 7,
              zero = 0: both 32-bit halves move, independently and backwards — flows.c:107-110,128

In ssl, hello and last the "role" of a record is its interface: the FIRST record of a script defines F (account.go:95 stores it
whole), so a script that starts on interface 2 has its records on interface 2 counted and those on interface 1 as side records.
No sequence is dropped: a family is exactly the sum of |S|^k scripts.

Two seeded families are too long to enumerate:

    capacity  2 000 scripts of 8..24 records around MAX_OBSERVED_INTERFACES (flows.c:79). The first record carries an observed
              list (nb_observed_intf in {0..6, 7, 255}, entries from the pool of nine interfaces 1..9, duplicates included,
              directions in {0..3}); side records follow on a seeded permutation of the pool, one to three directions each out of
              {0, 1, 2, 3, 7}, counted records in between. Even scripts ("listed"): the earliest side interfaces are already in the
              first record's list, so they append nothing and the list still has room when the SIXTH distinct side interface
              arrives — the last of the seven candidates the kernels keep — and is full for the seventh (a seventh can never find
              room: each of the six before it is in the list, that is the written argument of csrc/nfagg_dedup.hip:25-28; these
              scripts are the closest a flow gets). Odd scripts ("between"): an interface is appended with one direction, other
              interfaces then fill the list, and the interface's second direction arrives at a full list — flows.c:79 returns
              before the search, the direction must NOT become BOTH.
    wave      64 scripts of exactly 64 records over intf's symbols plus interfaces 3..8: in the flow-major layout script s is
              records [64 s, 64 s + 64) — one wave of 64 lanes holds a whole flow and every lane hits one slot.

Layouts are index arrays into a family's records (which are stored flow-major); each keeps every script's own order."""
import itertools
import zlib

import numpy as np

import keycraft as kc
from oracle.oracle import FLOW_RECORD

EXHAUSTIVE = ("intf", "ssl", "hello", "last")
SEEDED = ("capacity", "wave")
FAMILIES = EXHAUSTIVE + SEEDED
MAX_RECORDS = 50_000

END_A, END_B = (1 << 32) + 5, 7
SSL_VERSIONS = (0, 0x0303, 0x0304)
CIPHERS, KEY_SHARES = (0, 0x1301, 0xc02f), (0, 0x001d, 0x0017)
LAST_CLASSES = ((0, 0, 0), (46, 50, END_A), (8, 1, END_B))           # (dscp, sampling, end) of zero, a, b
POOL = np.arange(1, 10)                                              # capacity's nine interfaces
CAP_SCRIPTS, WAVE_SCRIPTS, WAVE_LEN = 2000, 64, 64

# symbol k of a family -> the fields it sets (the tables the records are built from AND re-derived by)
SYMBOLS = {
    "intf": [dict(if_index_first_seen=i, direction_first_seen=d) for i in (0, 1, 2) for d in (0, 1)],
    "ssl": [dict(if_index_first_seen=i, ssl_version=v) for i in (1, 2) for v in SSL_VERSIONS],
    "hello": [dict(if_index_first_seen=i, tls_types=t, tls_cipher_suite=c, tls_key_share=k)
              for i in (1, 2) for t in (1, 2) for c, k in zip(CIPHERS, KEY_SHARES)],
    "last": [dict(if_index_first_seen=i, dscp=d, sampling=s, end=e) for i in (1, 2) for d, s, e in LAST_CLASSES],
}
MAX_LEN = {"intf": 5, "ssl": 5, "hello": 3, "last": 5}
WAVE_SYMBOLS = SYMBOLS["intf"] + [dict(if_index_first_seen=i, direction_first_seen=d) for i in range(3, 9) for d in (0, 1)]
DIGITS = "0123456789abcdefghijklmnopqrstuvwxyz"


class Family:
    """recs: the records, flow-major (script 0's records, then script 1's, ...). script / pos: the script number of every record
    and its position in the script. start / length: where a script begins and how long it is. keys: (n_scripts, 40).
    symbols: the symbol table of an exhaustive or wave family (None for capacity); info: what a seeded builder designed."""

    def __init__(self, name, recs, script, pos, keys, symbols=None, info=None):
        self.name, self.recs, self.script, self.pos, self.keys, self.symbols, self.info = name, recs, script, pos, keys, symbols, info or {}
        self.n_scripts = len(keys)
        self.length = np.bincount(script, minlength=self.n_scripts)
        self.start = np.concatenate([[0], np.cumsum(self.length)[:-1]])
        assert np.array_equal(script, np.repeat(np.arange(self.n_scripts), self.length)), "records are stored flow-major"
        assert np.array_equal(pos, np.arange(len(recs)) - self.start[script])
        assert kc.distinct_flows(recs) == self.n_scripts, "one distinct flow key per script"
        assert len(recs) < MAX_RECORDS
        self._by_key = None

    def records_of(self, s):
        return self.recs[self.start[s]:self.start[s] + self.length[s]]

    def script_of_key(self, key):
        """The script whose flow has these key bytes (the first 39 count)."""
        if self._by_key is None:
            self._by_key = {bytes(k[:39]): s for s, k in enumerate(self.keys)}
        return self._by_key[bytes(np.ascontiguousarray(key).view(np.uint8).reshape(-1)[:39])]

    def scripts_of(self, records):
        """The script number of every record of an eviction."""
        raw = np.ascontiguousarray(records).view(np.uint8).reshape(len(records), 144)
        return np.array([self.script_of_key(raw[i, :40]) for i in range(len(raw))], dtype=np.int64)

    def describe(self, s):
        """The script as text: its symbol string where the family has symbols, its records' interface/direction otherwise."""
        r = self.records_of(s)["metrics"]
        if self.symbols is not None:
            return "%s script %d = '%s'" % (self.name, s, symbol_string(self.symbols, self.records_of(s)))
        first = "list %d %s/%s; " % (r["nb_observed_intf"][0], r["observed_intf"][0].tolist(), r["observed_direction"][0].tolist())
        return "%s script %d = %s%s" % (self.name, s, first, " ".join("%d/%d" % (i, d) for i, d in zip(r["if_index_first_seen"], r["direction_first_seen"])))


def symbol_numbers(symbols, recs):
    """The symbol of every record re-derived from the RECORDS (not from what the builder meant to write): exactly one must match."""
    m = recs["metrics"]
    out, hits = np.full(len(recs), -1, dtype=np.int64), np.zeros(len(recs), dtype=np.int64)
    for k, sym in enumerate(symbols):
        ok = np.ones(len(recs), dtype=bool)
        for f, v in sym.items():
            ok &= m[f] == v
        out[ok] = k
        hits += ok
    assert (hits == 1).all(), "a record matches no symbol, or several"
    return out


def symbol_string(symbols, recs):
    """One digit per record of a script."""
    return "".join(DIGITS[k] for k in symbol_numbers(symbols, recs))


def _keys(name, n):
    """n distinct, valid flow keys (byte 39 zero: Rec::canonicalize leaves them alone) from keycraft's builder, one target hash each."""
    rng = np.random.default_rng(zlib.crc32(("dedupcraft " + name).encode()))
    return kc.craft(kc._distinct(rng, n), rng)


def _blank(script, pos, keys):
    """The plain record of every (script, position): key, one packet, 100 bytes, IPv4, ACK, start 1000, end 2001 + position, counted on interface 1."""
    recs = np.zeros(len(script), dtype=FLOW_RECORD)
    recs.view(np.uint8).reshape(len(recs), 144)[:, :39] = keys[script, :39]
    m = recs["metrics"]
    m["start"], m["end"] = 1000, 2001 + pos
    m["bytes"], m["packets"], m["eth_protocol"], m["flags"] = 100, 1, 0x0800, 0x10
    m["if_index_first_seen"] = 1
    return recs


def _from_symbols(name, symbols, seqs):
    """seqs: one array (n_k, k) of symbol numbers per length."""
    script = np.concatenate([np.repeat(np.arange(len(q)), q.shape[1]) + off
                             for q, off in zip(seqs, np.cumsum([0] + [len(q) for q in seqs[:-1]]))])
    pos = np.concatenate([np.tile(np.arange(q.shape[1]), len(q)) for q in seqs])
    sym = np.concatenate([q.reshape(-1) for q in seqs])
    keys = _keys(name, sum(len(q) for q in seqs))
    recs = _blank(script, pos, keys)
    for field in sorted({f for s in symbols for f in s}):
        recs["metrics"][field] = np.array([s[field] for s in symbols], dtype=np.uint64)[sym]
    return Family(name, recs, script, pos, keys, symbols)


def exhaustive(name):
    symbols = SYMBOLS[name]
    seqs = [np.array(list(itertools.product(range(len(symbols)), repeat=k)), dtype=np.int64) for k in range(1, MAX_LEN[name] + 1)]
    return _from_symbols(name, symbols, seqs)


def wave():
    rng = np.random.default_rng(zlib.crc32(b"dedupcraft wave symbols"))
    return _from_symbols("wave", WAVE_SYMBOLS, [rng.integers(0, len(WAVE_SYMBOLS), size=(WAVE_SCRIPTS, WAVE_LEN))])


def _capacity_script(rng, half):
    """One script of the capacity family: (first record's nb, list entries, list directions, F, [(interface, direction), ...] of
    the records after the first, what was designed)."""
    F = 0 if rng.integers(0, 8) == 0 else int(rng.choice(POOL))
    sides = [int(x) for x in rng.permutation(POOL) if x != F]                      # eight or nine side interfaces in arrival order
    dirs = lambda k: [int(d) for d in rng.choice([0, 1, 2, 3, 7], size=k)]          # with repeats: "the same direction twice, then a third"
    intf = rng.choice(POOL, size=6)                                                 # entries past nb are noise the merge must not read
    info = {"half": half, "F": F}
    if half == 0:
        # "listed": nb entries drawn (with duplicates) from the earliest side interfaces — they are found, nothing is appended
        nb = int(rng.choice([1, 2, 3, 4, 5, 5, 4, 3, 0, 6, 7, 255]))
        k = min(nb, 6)
        intf[:k] = rng.choice(sides[:5], size=k)
        firsts = [(x, dirs(1)[0]) for x in sides]
        later = [(x, d) for x in sides for d in dirs(int(rng.integers(0, 3)))]
    else:
        # "between": X is appended with one direction, 5 - nb fresh interfaces fill the list, X's other direction finds it full
        nb = int(rng.integers(0, 6))
        intf[:nb] = rng.choice(sides[6:], size=nb)                                  # listed interfaces arrive late or never
        X, fill = sides[0], sides[1:6 - nb]
        d1 = int(rng.choice([0, 1]))
        firsts = [(X, d1)] + [(x, dirs(1)[0]) for x in fill] + [(X, 1 - d1)] + [(x, dirs(1)[0]) for x in sides[6 - nb:]]
        later = [(x, d) for x in sides[1:] for d in dirs(int(rng.integers(0, 3)))]
        info.update(X=X, d1=d1)
    n_total = int(rng.integers(8, 25))
    body = list(firsts)
    for ev in later:                                                                # further directions: anywhere after the designed part
        body.insert(int(rng.integers(len(firsts) if half else 1, len(body) + 1)), ev)
    body = body[:n_total - 1 - int(rng.integers(1, 4))]                             # room for one to three counted records
    while len(body) < n_total - 1:
        body.insert(int(rng.integers(0, len(body) + 1)), (F, int(rng.integers(0, 2))))
    return nb, intf, rng.integers(0, 4, size=6), F, body, info


def capacity():
    rng = np.random.default_rng(zlib.crc32(b"dedupcraft capacity scripts"))
    plans = [_capacity_script(rng, s % 2) for s in range(CAP_SCRIPTS)]
    length = np.array([1 + len(p[4]) for p in plans])
    script = np.repeat(np.arange(CAP_SCRIPTS), length)
    pos = np.arange(len(script)) - np.repeat(np.concatenate([[0], np.cumsum(length)[:-1]]), length)
    keys = _keys("capacity", CAP_SCRIPTS)
    recs = _blank(script, pos, keys)
    m = recs["metrics"]
    at = 0
    for nb, intf, odir, F, body, _ in plans:
        m["if_index_first_seen"][at], m["direction_first_seen"][at] = F, 0
        m["nb_observed_intf"][at], m["observed_intf"][at], m["observed_direction"][at] = nb, intf, odir
        n = len(body)
        m["if_index_first_seen"][at + 1:at + 1 + n] = [x for x, _ in body]
        m["direction_first_seen"][at + 1:at + 1 + n] = [d for _, d in body]
        at += 1 + n
    return Family("capacity", recs, script, pos, keys, None, {"plans": [p[5] for p in plans]})


_cache = {}


def family(name):
    """The family of that name, built once per process. Treat its arrays as read-only."""
    if name not in _cache:
        _cache[name] = exhaustive(name) if name in EXHAUSTIVE else {"capacity": capacity, "wave": wave}[name]()
    return _cache[name]


# ---------------------------------------------------------------- layouts: arrival orders that keep every script's own order
def flow_major(fam):
    """A script's records are adjacent (the order the records are stored in)."""
    return np.arange(len(fam.recs))


def round_major(fam):
    """Round j holds the j-th record of every script that has one, scripts in ascending order. Returns (order, bounds): round j is
    order[bounds[j]:bounds[j + 1]]."""
    order = np.lexsort((fam.script, fam.pos))
    bounds = np.concatenate([[0], np.cumsum(np.bincount(fam.pos))])
    return order, bounds


def shuffled(fam, seed=1):
    """A seeded merge of the scripts: the slots of a random permutation that fall to a script are filled in the script's order."""
    perm = np.random.default_rng(seed).permutation(len(fam.recs))
    # position i of the arrival order belongs to script fam.script[perm[i]]; the t-th position of a script takes its t-th record
    owner = fam.script[perm]
    nth = np.empty(len(perm), dtype=np.int64)
    by_owner = np.argsort(owner, kind="stable")
    nth[by_owner] = np.arange(len(perm)) - fam.start[owner[by_owner]]
    return fam.start[owner] + nth
