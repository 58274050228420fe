"""Flow keys with CHOSEN 64-bit key hashes (a helper module, no fixtures).

The key hash (csrc/nfagg_hash.h key_hash) is public and every step of it is a bijection of 64-bit words:
    h = seed;  for w in words: h = (rotl(h, 27) ^ w) * kMul;  return fmix64(h)
`x ^= x >> 33` is its own inverse (33 + 33 > 64), the three multipliers are odd and have inverses modulo 2^64, a rotation is undone
by the opposite one. So for ANY target hash and any choice of words 0, 1, 2 and 4 there is exactly one word 3 that gives it: run the
hash forwards over words 0..2, run it backwards from the target over fmix64 and word 4, and word 3 is what joins the two ends.
The seeded streams only ever hold keys whose hashes are effectively random; with this, a test gives the fold two flows with one
hash, hundreds of flows with one home slot, or a hash on a field boundary — in microseconds per key."""
import numpy as np

M64 = (1 << 64) - 1
K_MUL = 0x9E3779B97F4A7C15
K_SEED = 0x6E66616767206B31                    # "nfagg k1"
F1, F2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
K_MUL_INV, F1_INV, F2_INV = (pow(c, -1, 1 << 64) for c in (K_MUL, F1, F2))
assert all((a * b) & M64 == 1 for a, b in ((K_MUL, K_MUL_INV), (F1, F1_INV), (F2, F2_INV)))

_u = np.uint64


def _rot(x, r):
    """rotl by r on uint64 arrays (rotl by 37 = rotr by 27)."""
    return (x << _u(r)) | (x >> _u(64 - r))


def _fmix(x):
    x = x ^ (x >> _u(33)); x = x * _u(F1)
    x = x ^ (x >> _u(33)); x = x * _u(F2)
    return x ^ (x >> _u(33))


def _fmix_inv(x):
    x = x ^ (x >> _u(33)); x = x * _u(F2_INV)
    x = x ^ (x >> _u(33)); x = x * _u(F1_INV)
    return x ^ (x >> _u(33))


def as_words(keys):
    """(n, 40) uint8 keys (or anything with 40 bytes per row) -> (n, 5) little-endian uint64 words, byte 39 forced to zero."""
    b = np.ascontiguousarray(keys).view(np.uint8).reshape(-1, 40).copy()
    b[:, 39] = 0
    return b.view("<u8").reshape(-1, 5)


def key_hash(words):
    """csrc/nfagg_hash.h key_hash restated, vectorised: words = (n, 5) little-endian uint64, byte 39 zero. Returns (n,) uint64."""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 5)
    assert not (w[:, 4] >> _u(56)).any(), "byte 39 is not part of the key: it must be zero here"
    h = np.full(len(w), K_SEED, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for i in range(5):
            h = (_rot(h, 27) ^ w[:, i]) * _u(K_MUL)
        return _fmix(h)


def craft(targets, rng, fixed=None):
    """One 40-byte key per 64-bit target hash: (n, 40) uint8, key_hash(key) == target, byte 39 zero, all keys distinct.
    Words 0, 1, 2 and the low 56 bits of word 4 are drawn from rng (full width: the keys look like IPv6 flows with arbitrary
    ports), word 3 is solved. fixed = {word index in (0, 1, 2, 4): value or (n,) array} pins words instead of drawing them."""
    t = np.ascontiguousarray(np.asarray(targets, dtype=np.uint64).reshape(-1))
    n = len(t)
    w = rng.integers(0, 1 << 64, size=(n, 5), dtype=np.uint64)
    for k, v in (fixed or {}).items():
        assert k in (0, 1, 2, 4), "word 3 is the one that is solved"
        w[:, k] = np.asarray(v, dtype=np.uint64)
    w[:, 4] &= _u((1 << 56) - 1)
    with np.errstate(over="ignore"):
        h3 = np.full(n, K_SEED, dtype=np.uint64)
        for i in range(3):
            h3 = (_rot(h3, 27) ^ w[:, i]) * _u(K_MUL)                 # the state after words 0..2
        h5 = _fmix_inv(t)                                              # the state after word 4
        h4 = _rot((h5 * _u(K_MUL_INV)) ^ w[:, 4], 37)                  # ... after word 3
        w[:, 3] = (h4 * _u(K_MUL_INV)) ^ _rot(h3, 27)
    assert np.array_equal(key_hash(w), t)
    keys = np.ascontiguousarray(w).view(np.uint8).reshape(n, 40)
    assert not keys[:, 39].any()
    assert len(np.unique(keys, axis=0)) == n, "crafted keys must be distinct flows"
    return keys


# ---------------------------------------------------------------- addresses with chosen ip_hash values
IP_SEEDS = (0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89)


def ip_hash(lo, hi, seed_index):
    """csrc/nfagg_hash.h ip_hash restated, vectorised: lo / hi = the address's little-endian 64-bit words. Returns uint64."""
    lo, hi = np.asarray(lo, dtype=np.uint64), np.asarray(hi, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = (_rot(_u(IP_SEEDS[seed_index & 3]), 27) ^ lo) * _u(K_MUL)
        return _fmix((_rot(h, 27) ^ hi) * _u(K_MUL))


def ip_words(addrs):
    """(n, 16) uint8 addresses -> (lo, hi) little-endian uint64 words."""
    w = np.ascontiguousarray(addrs, dtype=np.uint8).reshape(-1, 16).view("<u8")
    return w[:, 0].copy(), w[:, 1].copy()


def craft_ip(targets, seed_index, rng):
    """One 16-byte address per 64-bit target: (n, 16) uint8 with ip_hash(address, seed_index) == target, all addresses distinct.
    For any lower word the hash is a bijection of the upper word: the lower word is drawn from rng, the upper one solved (the
    hash run forwards over the lower word, backwards from the target over fmix64 and the last multiplication). Equal targets get
    different addresses, because their lower words differ."""
    t = np.ascontiguousarray(np.asarray(targets, dtype=np.uint64).reshape(-1))
    lo = _distinct(rng, len(t))
    with np.errstate(over="ignore"):
        h1 = (_rot(_u(IP_SEEDS[seed_index & 3]), 27) ^ lo) * _u(K_MUL)
        hi = (_fmix_inv(t) * _u(K_MUL_INV)) ^ _rot(h1, 27)
    assert np.array_equal(ip_hash(lo, hi, seed_index), t)
    return np.ascontiguousarray(np.stack([lo, hi], axis=1).astype("<u8")).view(np.uint8).reshape(len(t), 16)


def _key_column(recs):
    """The 40 key bytes of every record with byte 39 zeroed, as one opaque 40-byte column (sorts much faster than 39 columns)."""
    raw = np.ascontiguousarray(np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), 144)[:, :40])
    raw[:, 39] = 0
    return raw.view(np.dtype((np.void, 40))).reshape(-1)


def flow_ranks(recs):
    """The flows of a stream (distinct key bytes 0..38), hottest first: (inverse, order) where inverse[i] is the flow number of
    record i and order[r] the flow number of rank r (most records first; ties in order of the key bytes)."""
    _, inverse, counts = np.unique(_key_column(recs), return_inverse=True, return_counts=True)
    return inverse.reshape(-1), np.argsort(-counts, kind="stable")


def remap(recs, ranks, keys):
    """A copy of recs in which every record of the flow of rank ranks[k] carries keys[k] in its key bytes 0..38. Byte 39 (the pad
    that is no part of the identity; stream variant 1 dirties it on purpose) and everything else stay as the stream made them."""
    keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 40)
    ranks = np.asarray(ranks).reshape(-1)
    assert len(ranks) == len(keys) and len(np.unique(ranks)) == len(ranks)
    inverse, order = flow_ranks(recs)
    assert ranks.max() < len(order), "the stream has only %d flows" % len(order)
    new_key = np.full(len(order), -1, dtype=np.int64)
    new_key[order[ranks]] = np.arange(len(keys))
    out = np.ascontiguousarray(recs).copy()
    raw = out.view(np.uint8).reshape(len(out), 144)
    k = new_key[inverse]
    hit = k >= 0
    raw[hit, :39] = keys[k[hit], :39]
    return out


# ---------------------------------------------------------------- the constants the families are built around, read from the source
def fold_constants():
    """Probe windows and cache sizes of the LDS caches, and the number of spill partitions, parsed from csrc/ (a family built
    around a guessed window would stop reaching its branch the day the window changes). The text is read, not the binary: this is
    the value of the default build. NF_PART_PROBE can be overridden on the compiler's command line (it sits in an #ifndef); a
    library built that way has another window than the one returned here."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "netobserv-ebpf-agent_amd", "csrc")

    def grab(fname, pattern):
        with open(os.path.join(csrc, fname)) as f:
            m = re.search(pattern, f.read(), re.M)
        assert m, (fname, pattern)
        return int(m.group(1))

    c = {
        "kProbe": grab("nfagg_ingest_part.hip", r"^#define NF_PART_PROBE (\d+)"),
        "kEntries": grab("nfagg_ingest_part.hip", r"^constexpr int kEntries = (\d+);"),
        "kCacheProbe": grab("nfagg_ingest_cached.hip", r"^constexpr int kCacheProbe = (\d+);"),
        "kDedupProbe": grab("nfagg_dedup_cached.hip", r"^constexpr int kProbe = (\d+);"),
        "kPartEntries": grab("nfagg_dedup_cached.hip", r"^constexpr int kPartEntries = (\d+);"),
        "kSpillParts": grab("nfagg_internal.h", r"^constexpr int kSpillParts = (\d+);"),
    }
    c["window"] = max(c["kProbe"], c["kCacheProbe"], c["kDedupProbe"])
    return c


# ---------------------------------------------------------------- the group hash of the metrics fold (csrc/nfagg_metrics.h)
def metrics_group_hash(grouping, src_class, dst_class, src_label=0xFFFF, dst_label=0xFFFF, direction=0xFF, layer=0, proto=0, is_ip=0):
    """met_hash(met_key_a, met_key_b) restated, vectorised over any of the key fields (the defaults are every dimension's "none").
    A = 1<<63 | g<<58 | dst_class<<29 | src_class; B = 1<<63 | g<<56 | is_ip<<50 | proto<<42 | layer<<40 | direction<<32 |
    dst_label<<16 | src_label; hash = fmix64((rotl(A * kMul, 27) ^ B) * kMul)."""
    f = [np.asarray(x, dtype=np.uint64) for x in (src_class, dst_class, src_label, dst_label, direction, layer, proto, is_ip)]
    g, mark = _u(grouping), _u(1 << 63)
    a = mark | (g << _u(58)) | (f[1] << _u(29)) | f[0]
    b = mark | (g << _u(56)) | (f[7] << _u(50)) | (f[6] << _u(42)) | (f[5] << _u(40)) | (f[4] << _u(32)) | (f[3] << _u(16)) | f[2]
    with np.errstate(over="ignore"):
        return _fmix((_rot(a * _u(K_MUL), 27) ^ b) * _u(K_MUL))


def _grab(fname, pattern):
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "netobserv-ebpf-agent_amd", "csrc")
    with open(os.path.join(csrc, fname)) as f:
        m = re.search(pattern, f.read(), re.M)
    assert m, (fname, pattern)
    return int(m.group(1))


def metrics_constants():
    """The sizes the metrics fold's families are built around, parsed from csrc/ like fold_constants()."""
    return {"kMetLdsSlots": _grab("nfagg_metrics.hip", r"\bkMetLdsSlots = (\d+)"), "kMetLdsProbe": _grab("nfagg_metrics.hip", r"\bkMetLdsProbe = (\d+)"),
            "kMetFlowsPerBlock": _grab("nfagg_metrics.hip", r"^constexpr uint64_t kMetFlowsPerBlock = (\d+);"),
            "kMetMinSlots": _grab("nfagg_metrics.h", r"\bkMetMinSlots = (\d+)")}


def partition_constants():
    """Tile size, the scan's chunk of tiles and the grid cap of the stable partition, parsed from csrc/nfagg_partition.hip."""
    f = "nfagg_partition.hip"
    c = {"kPartBlock": _grab(f, r"^constexpr int kPartBlock = (\d+);"), "kPartRounds": _grab(f, r"^constexpr int kPartRounds = (\d+);"),
         "kMaxShards": _grab(f, r"^constexpr int kMaxShards = (\d+);"),
         "scan_chunk": _grab(f, r"for \(uint32_t t0 = 0; t0 < n_tiles; t0 \+= (\d+)\)"), "grid_cap": _grab(f, r"const unsigned grid = n_tiles < (\d+)u")}
    c["tile"] = c["kPartBlock"] * c["kPartRounds"]
    return c


# ---------------------------------------------------------------- families of target hashes
FAMILIES = ("same64", "bit0", "one_home_ones", "one_home_m5", "same_fp", "cache_wrap", "edge", "one_bit")
ONE_HOME_K = 300
SAME64_GROUPS = (2, 2, 2, 3, 3, 3, 40, 40)
N_RECORDS, N_FLOWS, COLD_RANK = 60_000, 3_000, 1_500


def _distinct(rng, n, bits=64):
    while True:
        v = rng.integers(0, 1 << bits, size=n, dtype=np.uint64)
        if len(np.unique(v)) == n:
            return v


def family_targets(name, rng, mask, consts):
    """The target hashes of a family (see each branch) for a table of mask + 1 slots."""
    bits = int(mask).bit_length()
    assert mask == (1 << bits) - 1 and 10 <= bits <= 21       # the fold's tables have 2^16..2^21 slots, the map merge's join 2^10 and up
    win, ent = consts["window"], consts["kEntries"]
    if name == "same64":                      # groups of flows with ONE hash: every full-key compare behind a hash match
        return np.repeat(_distinct(rng, len(SAME64_GROUPS)), SAME64_GROUPS)
    if name == "bit0":                        # h and h ^ 1: one LDS cache entry (the caches store h | 1), two home slots
        h = _distinct(rng, 50, 63) << _u(1)
        return np.stack([h, h | _u(1)], axis=1).reshape(-1)
    if name in ("one_home_ones", "one_home_m5"):
        # K flows with equal low 21 bits (one home slot, one partition, one sub-partition in every table up to 2^21 slots) and
        # distinct upper bits: a probe chain of K slots, from the table's LAST slot round to slot 0 / ending a few slots before it
        low = (1 << 21) - 1 if name == "one_home_ones" else (((1 << 21) - 1) & ~int(mask)) | (int(mask) - 5)
        return (_distinct(rng, ONE_HOME_K, 43) << _u(21)) | _u(low)
    if name == "same_fp":
        # bits 18..63 equal: ONE fingerprint (the `locked` / `ready` tags of all these flows are equal) and one LDS home entry
        # ((h >> 40) & 1023), in 2 x window CONSECUTIVE home slots across a border of the pass-2 partitions (the top 8..11 bits of
        # the slot index: a multiple of slots / 256 is a border for every partition count)
        upper = int(rng.integers(0, 1 << 46)) << 18
        step = (mask + 1) >> 8
        border = ((upper & int(mask)) & ~((1 << 18) - 1)) | (int(rng.integers(1, min(1 << 18, mask + 1) // step)) * step)
        return np.array([upper | (border - win + k) for k in range(2 * win)], dtype=np.uint64)
    if name == "cache_wrap":                  # LDS home entries kEntries - 2 and kEntries - 1, 2 x window flows each: probing wraps to entry 0
        out = []
        for e in (ent - 2, ent - 1):
            r = _distinct(rng, 2 * win)
            out.append((r & ~_u((ent - 1) << 40)) | _u(e << 40))
        return np.concatenate(out)
    if name == "edge":                        # free marker 0, the busy marker 2 (hash 2 is stored as 3), all-ones index fields; a few sharing 0 / all ones
        return np.array([0, 1, 2, 3, 1 << 63, M64 - 1, M64, 0, 0, M64, M64], dtype=np.uint64)
    raise KeyError(name)


def shard_edge_targets(rng, n_shards, per_value=4):
    """Hashes whose upper 32 bits sit on both sides of every boundary of shard_of_hash's multiply-shift ((h >> 32) * n >> 32):
    ceil(k 2^32 / n) - 1 and ceil(k 2^32 / n) for k = 1..n - 1, plus 0 and 2^32 - 1; the lower 32 bits are random."""
    hi = {0, (1 << 32) - 1}
    for k in range(1, n_shards):
        c = -((-k << 32) // n_shards)
        hi |= {c - 1, c}
    hi = np.repeat(np.array(sorted(hi), dtype=np.uint64), per_value)
    return (hi << _u(32)) | rng.integers(0, 1 << 32, size=len(hi), dtype=np.uint64)


def hot_and_cold_ranks(k, rng):
    """Half of a family's flows become the stream's hottest (they live in the LDS caches), half cold ones of a few records each
    (spilled or bypassed) — dealt at random, so that a group of equal hashes has flows of both kinds."""
    ranks = np.concatenate([np.arange(k // 2), COLD_RANK + np.arange(k - k // 2)])
    return ranks[rng.permutation(k)]


def one_bit_keys(rng):
    """No crafting: a random 39-byte base key and its 312 single-bit neighbours (313 flows that differ in ONE bit of ONE of the five
    key words each). Returns (313, 40) uint8, base first, byte 39 zero."""
    base = rng.integers(0, 256, size=40, dtype=np.uint8)
    base[39] = 0
    keys = np.tile(base, (313, 1))
    for b in range(312):
        keys[1 + b, b // 8] ^= np.uint8(1 << (b % 8))
    return keys


def apply_family(base, name, mask, consts=None):
    """The base stream with one family planted in it. Returns (records, keys planted (k, 40), their target hashes or None)."""
    import zlib
    consts = consts or fold_constants()
    rng = np.random.default_rng(zlib.crc32(name.encode()) + int(mask))
    if name == "one_bit":
        # every flow of the stream gets a full-width key: the 313 neighbours (half hot, half cold), then eight more flows that ARE
        # the base flow — its key bytes 0..38 and byte 39 with one bit flipped each — and random keys for all the others
        inverse, order = flow_ranks(base)
        n = len(order)
        keys = rng.integers(0, 256, size=(n, 40), dtype=np.uint8)
        keys[:, 39] = 0
        nb = one_bit_keys(rng)
        ranks = hot_and_cold_ranks(len(nb), rng)
        keys[ranks] = nb
        pad_ranks = 400 + np.arange(8)
        keys[pad_ranks] = nb[0]
        out = remap(base, np.arange(n), keys)
        raw = out.view(np.uint8).reshape(len(out), 144)
        for b, r in enumerate(pad_ranks):
            raw[inverse == order[r], 39] = np.uint8(1 << b)
        return out, nb, None
    targets = family_targets(name, rng, mask, consts)
    keys = craft(targets, rng)
    return remap(base, hot_and_cold_ranks(len(keys), rng), keys), keys, targets


def distinct_flows(recs):
    """len(np.unique(keys)): the flows of a stream by key bytes 0..38."""
    return len(np.unique(_key_column(recs)))


def apply_shard_edge(base, n_shards):
    """The base stream with shard_edge_targets(n_shards) planted, half hot and half cold. Returns (records, keys, targets)."""
    rng = np.random.default_rng(7000 + n_shards)
    targets = shard_edge_targets(rng, n_shards)
    keys = craft(targets, rng)
    return remap(base, hot_and_cold_ranks(len(keys), rng), keys), keys, targets


def shard_formula(recs, n_shards):
    """((h >> 32) * n) >> 32 of every record's key, in Python integers."""
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), 144)[:, :40]
    return np.array([((int(h) >> 32) * n_shards) >> 32 for h in key_hash(as_words(raw))], dtype=np.int64)
