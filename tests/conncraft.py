"""The conversation fold restated over arrays, and the searches for crafted connection hashes (numpy only, no import of the
product). tests/conntrack_ref.py hashes and folds one flow at a time with Python integers; that is the reference of the small
streams. Here the same FNV-64a over the same gob messages runs over arrays, for streams of a million flows and for searches over
2^22 .. 2^25 tuples, restricted to inputs whose messages have ONE LENGTH PER CLASS:

    address   IPv4 10.B.C.D with B, C, D in 100..255: always 14 characters, message 11 0c 00 0e "10.BBB.CCC.DDD"
    port      1024..65535: always 05 06 00 fe hi lo
    protocol  6 / 17 (03 06 00 pp) and 132 (04 06 00 ff 84)

fold() restates nfagg_conn_fold with numpy's unique / ufunc.at over such a stream and returns what conntrack_ref.fold returns.
tests/test_conncraft_cpu.py holds both restatements against each other and against nfagg_conn_hash.

The searches (tests/golden/gen_conntrack_crafted.py writes their results to tests/golden/conntrack_crafted.json):
    search_homes()    over the space of conntrack_collisions.json (10.1.2.3 -> 10.9.8.7, 2 048 x 2 048 ports, TCP): connections
                      with one home slot in the 1 024-slot table, and connections whose home is one of the last three slots of
                      the 1 024-slot and of the 8 192-slot table
    search_word0()    over 2^25 tuples of the fixed-length class (8 x 4 addresses, 1 024 x 1 024 ports, TCP): pairs of
                      connections whose totals share the upper 32 bits, the table's first key word, AND the 1 024-slot home. A
                      birthday on 32 + 10 bits: 2^25 tuples hold about 2^50 / 2^43 = 128 such pairs."""
import numpy as np

import ipfix_ref

M64 = (1 << 64) - 1
OFFSET, PRIME = 0xcbf29ce484222325, 0x100000001b3
NO_IDX = 0xFFFFFFFF
FIN = 0x01
PROTO_MSG = {6: bytes([3, 6, 0, 6]), 17: bytes([3, 6, 0, 17]), 132: bytes([4, 6, 0, 0xff, 132])}
PORT_HEAD = bytes([5, 6, 0, 0xfe])
V4_PREFIX = bytes(10) + b"\xff\xff"

# nfagg_conn_partial as include/nfagg.h lays it out (tests/test_conncraft_cpu.py compares it with the product's dtype)
CONN_PARTIAL = np.dtype([("hash_total", "<u8"), ("first_hash_a", "<u8"), ("first_idx", "<u4"), ("last_idx", "<u4"), ("first_fin_idx", "<u4"),
                         ("flags_or", "<u4"), ("flows", "<u8", (2,)), ("bytes", "<u8", (2,)), ("packets", "<u8", (2,)), ("start_ms_min", "<i8"),
                         ("end_ms_max", "<i8"), ("pad_", "<u8", (4,))])


def fnv(data: bytes, h: int = OFFSET) -> int:
    """The plain byte-by-byte FNV-64a."""
    for b in data:
        h = ((h ^ b) * PRIME) & M64
    return h


def vfnv(h, byte):
    """One FNV-64a step over arrays: h uint64, byte any unsigned integer array below 256."""
    with np.errstate(over="ignore"):
        return (h ^ byte.astype(np.uint64)) * np.uint64(PRIME)


def vfnv_be64(h, w):
    for k in range(7, -1, -1):
        h = vfnv(h, (w >> np.uint64(8 * k)) & np.uint64(255))
    return h


def vfmix64(x):
    """MurmurHash3's finalizer over a uint64 array (conntrack_streams.fmix64 is the scalar)."""
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xff51afd7ed558ccd)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xc4ceb9fe1a85ec53)
        return x ^ (x >> np.uint64(33))


def vhome(total, slots=1024):
    return (vfmix64(total) & np.uint64(slots - 1)).astype(np.int64)


def str_msg(text: str) -> bytes:
    return bytes([3 + len(text), 0x0c, 0, len(text)]) + text.encode()


def _ports(h, port):
    port = np.asarray(port).astype(np.uint64)
    assert ((port >= 1024) & (port <= 65535)).all(), "ports of the fixed-length class are 1024..65535"
    for b in PORT_HEAD:
        h = vfnv(h, np.uint64(b))
    return vfnv(vfnv(h, port >> np.uint64(8)), port & np.uint64(255))


def side_hash(addr_bytes, port):
    """hashA / hashB of (address, port) over arrays. addr_bytes: (..., 4) uint8 or the record's (..., 16) v4-mapped form."""
    a = np.asarray(addr_bytes)
    if a.shape[-1] == 16:
        assert (a[..., :12] == np.frombuffer(V4_PREFIX, dtype=np.uint8)).all(), "addresses of the fixed-length class are v4-mapped"
        a = a[..., 12:]
    assert a.shape[-1] == 4 and (a[..., 0] == 10).all() and (a[..., 1:] >= 100).all(), "addresses of the fixed-length class are 10.B.C.D, B, C, D >= 100"
    h = np.full(a.shape[:-1], fnv(str_msg("10.000.000.000")[:7]), dtype=np.uint64)           # 11 0c 00 0e "10."
    for k in (1, 2, 3):
        v = a[..., k].astype(np.uint64)
        for digit in (v // np.uint64(100), v // np.uint64(10) % np.uint64(10), v % np.uint64(10)):
            h = vfnv(h, digit + np.uint64(0x30))
        if k < 3:
            h = vfnv(h, np.uint64(0x2e))
    return _ports(h, port)


def fixed_side_hash(addr_text: str, port):
    """hashA / hashB of one address, given as net.IP.String() prints it, over an array of ports of the fixed-length class."""
    port = np.asarray(port)
    return _ports(np.full(port.shape, fnv(str_msg(addr_text)), dtype=np.uint64), port)


def totals(hash_a, hash_b, proto):
    """hashTotal: the common group's hash (Proto), the smaller endpoint hash, the other, each as eight big-endian bytes."""
    hash_a, hash_b = np.asarray(hash_a, dtype=np.uint64), np.asarray(hash_b, dtype=np.uint64)
    proto = np.broadcast_to(np.asarray(proto), hash_a.shape)
    assert np.isin(proto, list(PROTO_MSG)).all(), "protocols of the fixed-length class are 6, 17 and 132"
    lut = np.zeros(256, dtype=np.uint64)
    for p, msg in PROTO_MSG.items():
        lut[p] = fnv(fnv(msg).to_bytes(8, "big"))
    t = lut[proto]
    t = vfnv_be64(t, np.minimum(hash_a, hash_b))
    return vfnv_be64(t, np.maximum(hash_a, hash_b))


def plain_hashes(src: str, sport: int, dst: str, dport: int, proto: int):
    """(hashA, hashB, hashTotal) of one tuple by the plain FNV, for the generator's re-check of what the searches found."""
    def uint_msg(v):
        return bytes([3, 6, 0, v]) if v < 128 else bytes([4, 6, 0, 0xff, v]) if v < 256 else bytes([5, 6, 0, 0xfe, v >> 8, v & 255])
    a, b, c = fnv(str_msg(src) + uint_msg(sport)), fnv(str_msg(dst) + uint_msg(dport)), fnv(uint_msg(proto))
    return a, b, fnv(c.to_bytes(8, "big") + min(a, b).to_bytes(8, "big") + max(a, b).to_bytes(8, "big"))


# ---- records of the fixed-length class
def records(dtype, src4, sport, dst4, dport, proto, rng=None, eth=0x0800):
    """144-byte records (dtype: the product's FLOW_RECORD) from (n, 4) address bytes, ports and protocols. With an rng: bytes up to
    2^40 and zero, packets, flags (FIN, SYN_ACK and none among them, on every protocol) and times on both sides of 2^41."""
    n = len(sport)
    r = np.zeros(n, dtype=dtype)
    for side, a in (("src_ip", src4), ("dst_ip", dst4)):
        r["id"][side][:, 10:12] = 0xFF
        r["id"][side][:, 12:] = a
    r["id"]["src_port"], r["id"]["dst_port"], r["id"]["transport_protocol"] = sport, dport, proto
    r["metrics"]["eth_protocol"] = eth
    if rng is not None:
        m = r["metrics"]
        m["bytes"] = rng.integers(0, 1 << 40, n, dtype=np.uint64) * (rng.integers(0, 5, n) > 0)
        m["packets"] = rng.integers(0, 1 << 20, n, dtype=np.uint32) * (rng.integers(0, 5, n) > 0)
        m["flags"] = rng.choice(np.array([0, 0x10, 0x10, 0x11, 0x112, 0x01, 0x02, 0x8000], dtype=np.uint16), n)
        m["start_mono_time_ts"] = rng.integers(0, 1 << 42, n, dtype=np.uint64)
        m["end_mono_time_ts"] = rng.integers(0, 1 << 42, n, dtype=np.uint64)
    return r


def turned(r, mask):
    """The records under the mask turned round: the other direction of the same connection."""
    k = r["id"]
    for a, b in (("src_ip", "dst_ip"), ("src_port", "dst_port")):
        x, y = k[a].copy(), k[b].copy()
        k[a][mask], k[b][mask] = y[mask], x[mask]
    return r


def both_ways(r, rng):
    """Half of the records, at random, turned round."""
    return turned(r, rng.integers(0, 2, len(r)) > 0)


def distinct(dtype, n, rng=None, first=0):
    """n records of n distinct connections of the fixed-length class (number `first` onwards of 2^24 x 3 protocols)."""
    q = first + np.arange(n)
    src4 = np.stack([np.full(n, 10), 100 + (q >> 14) % 156, 100 + (q >> 7) % 128, 100 + q % 128], axis=1)
    dst4 = np.stack([np.full(n, 10), 200 + (q >> 21) % 56, np.full(n, 222), np.full(n, 111)], axis=1)
    proto = np.array([6, 17, 132])[(q >> 24) % 3]
    return records(dtype, src4, 2000 + q % 7, dst4, np.full(n, 4443), proto, rng)


def with_metrics(r, rng):
    """Random bytes, packets, flags and times, as records() draws them, over records that have their ids."""
    m = records(r.dtype, np.zeros((len(r), 4)), np.zeros(len(r)), np.zeros((len(r), 4)), np.zeros(len(r)), 0, rng)["metrics"]
    for f in ("bytes", "packets", "flags", "start_mono_time_ts", "end_mono_time_ts"):
        r["metrics"][f] = m[f]
    return r


def seeded_stream(dtype, n, seed, n_conns, discard_one_in=9):
    """n flows over at most n_conns connections of the fixed-length class (TCP, UDP and SCTP), both directions, random flags on
    every protocol; two flows in discard_one_in are ICMP or carry a non-IP ethertype and are discarded, and one more is a
    v4-mapped address under the IPv6 ethertype, which is tracked."""
    rng = np.random.default_rng(seed)
    pool = distinct(dtype, n_conns)
    pool["id"]["transport_protocol"] = rng.choice(np.array([6, 6, 17, 132], dtype=np.uint8), n_conns)
    recs = both_ways(with_metrics(pool[rng.integers(0, n_conns, n)], rng), rng)
    out = rng.integers(0, discard_one_in, n)
    recs["id"]["transport_protocol"][out == 0] = 1
    recs["metrics"]["eth_protocol"][out == 1] = 0x0806
    recs["metrics"]["eth_protocol"][out == 2] = 0x86DD
    return recs


def time_values(mono):
    """Timestamps before mono_now, equal to it, after it, 0 and 2^64 - 1; around one millisecond and one second either way (the
    nsec carry and borrow), and far enough before it that a clock near 1970 gives negative milliseconds."""
    near = [-4 * 10**12, -3 * 10**12, -5_000_000_001, -2_000_000_001, -10**9, -999_999_999, -1_000_001, -1_000_000, -1, 0, 1, 999_999, 1_000_000, 10**9 - 1, 10**9, 7 * 10**12]
    return sorted({(mono + d) & M64 for d in near} | {0, 1 << 63, M64})


def time_stream(dtype, mono, seed=0):
    """Connections of three flows each, interleaved (flow j of connection c is record j * C + c) and in both directions: for
    every (where the least start is, where the greatest end is) in first / middle / last, eight triples of distinct time_values,
    two of them from values more than two seconds before mono_now (under a clock below one second, all their times are negative).
    Returns (records, per connection (where_min, where_max))."""
    rng = np.random.default_rng(seed)
    vals = np.array(time_values(mono), dtype=np.uint64)
    signed = (vals - np.uint64(mono)).view(np.int64)                 # flow time is monotone in int64(ts - mono_now)
    early = np.flatnonzero(signed <= -2_000_000_001)
    where = [(a, b) for a in range(3) for b in range(3) for _ in range(8)]
    nc = len(where)
    r = distinct(dtype, nc, first=5000)
    r = np.concatenate([r, r, r])
    r["metrics"]["bytes"], r["metrics"]["packets"], r["metrics"]["flags"] = 1000 + np.arange(3 * nc), 1, 0x10
    for c, (a, b) in enumerate(where):
        for field, at, pick in (("start_mono_time_ts", a, np.argmin), ("end_mono_time_ts", b, np.argmax)):
            three = rng.choice(early if c % 8 < 2 else len(vals), 3, replace=False)
            best = int(three[pick(signed[three])])
            rest = [int(v) for v in three if v != best]
            order = rest[:at] + [best] + rest[at:]
            for j in range(3):
                r["metrics"][field][j * nc + c] = vals[order[j]]
    return turned(r, np.arange(3 * nc) % 2 == 1), where


# ---- the fold
def tracked(recs):
    eth, proto = recs["metrics"]["eth_protocol"], recs["id"]["transport_protocol"]
    return ((eth == 0x0800) | (eth == 0x86DD)) & ((proto == 6) | (proto == 17) | (proto == 132))


def fold(recs, now_unix_ns, mono_now_ns):
    """conntrack_ref.fold over arrays: (partials as a CONN_PARTIAL array in first_idx order, hash ids uint64[n], n_discarded).
    Every flow the filter keeps must be of the fixed-length class (asserted)."""
    n = len(recs)
    keep = tracked(recs)
    idx = np.flatnonzero(keep)
    k, m = recs["id"][idx], recs["metrics"][idx]
    ha, hb = side_hash(k["src_ip"], k["src_port"]), side_hash(k["dst_ip"], k["dst_port"])
    total = totals(ha, hb, k["transport_protocol"])
    ids = np.zeros(n, dtype=np.uint64)
    ids[idx] = total
    uniq, first, inv = np.unique(total, return_index=True, return_inverse=True)      # first: the first occurrence of each
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    conn = rank[inv.reshape(-1)]                                                     # per kept flow: its connection, in first_idx order
    first = first[order]
    nc = len(uniq)
    p = np.zeros(nc, dtype=CONN_PARTIAL)
    p["hash_total"], p["first_hash_a"], p["first_idx"] = uniq[order], ha[first], idx[first]
    last = np.zeros(nc, dtype=np.int64)
    np.maximum.at(last, conn, idx)
    p["last_idx"] = last
    tcp = k["transport_protocol"] == 6                                               # only TCP has the Flags key
    flags = m["flags"].astype(np.uint32)
    fin = np.full(nc, NO_IDX, dtype=np.int64)
    has_fin = tcp & ((flags & FIN) != 0)
    np.minimum.at(fin, conn[has_fin], idx[has_fin])
    p["first_fin_idx"] = fin
    flags_or = np.zeros(nc, dtype=np.uint32)
    np.bitwise_or.at(flags_or, conn[tcp], flags[tcp])
    p["flags_or"] = flags_or
    side = (ha != ha[first][conn]).astype(np.int64)
    for name, v in (("flows", np.ones(len(idx), dtype=np.uint64)), ("bytes", m["bytes"].astype(np.uint64)), ("packets", m["packets"].astype(np.uint64))):
        acc = np.zeros((nc, 2), dtype=np.uint64)
        with np.errstate(over="ignore"):
            np.add.at(acc, (conn, side), v)
        p[name] = acc
    start = ipfix_ref.flow_times(m["start_mono_time_ts"], now_unix_ns, mono_now_ns)[1].view(np.int64)
    end = ipfix_ref.flow_times(m["end_mono_time_ts"], now_unix_ns, mono_now_ns)[1].view(np.int64)
    lo, hi = np.full(nc, np.iinfo(np.int64).max), np.full(nc, np.iinfo(np.int64).min)
    np.minimum.at(lo, conn, start)
    np.maximum.at(hi, conn, end)
    p["start_ms_min"], p["end_ms_max"] = lo, hi
    return p, ids, int(n - len(idx))


# ---- the searches
SIDE = 2048
GOLDEN_SRC, GOLDEN_DST = "10.1.2.3", "10.9.8.7"


def _grid_totals(side_a, side_b, proto=6):
    a, b = np.meshgrid(side_a, side_b, indexing="ij")
    return totals(a.ravel(), b.ravel(), proto)


def search_homes(n_same=200, n_wrap_small=40, n_wrap_big=30):
    """Over the 2^22 tuples (10.1.2.3, 1024 + i) -> (10.9.8.7, 1024 + j), TCP. Returns a dict of the families and how many
    candidates each had."""
    ports = np.arange(1024, 1024 + SIDE)
    t = _grid_totals(fixed_side_hash(GOLDEN_SRC, ports), fixed_side_hash(GOLDEN_DST, ports))
    home = vhome(t, 1024)
    best = int(np.bincount(home, minlength=1024).argmax())
    same = np.flatnonzero(home == best)
    wrap_small = np.flatnonzero(home >= 1024 - 3)
    home_big = vhome(t, 8192)
    wrap_big = np.flatnonzero(home_big >= 8192 - 3)

    def tup(ix, home_of):
        return dict(src=GOLDEN_SRC, sport=1024 + int(ix) // SIDE, dst=GOLDEN_DST, dport=1024 + int(ix) % SIDE, proto=6, total="%x" % int(t[ix]), home=int(home_of[ix]))
    return dict(searched=int(t.size), home_slot=best,
                candidates=dict(same_home=int(len(same)), wrap_1024=int(len(wrap_small)), wrap_8192=int(len(wrap_big))),
                same_home=[tup(i, home) for i in same[:n_same]], wrap_1024=[tup(i, home) for i in wrap_small[:n_wrap_small]],
                wrap_8192=[tup(i, home_big) for i in wrap_big[:n_wrap_big]])


WORD0_SRC = [(10, 101, 102, 100 + k) for k in range(8)]
WORD0_DST = [(10, 201, 202, 100 + k) for k in range(4)]
WORD0_PORTS = 1024                                                  # 1024 .. 2047 on either side


def _word0_chunk(s, d):
    ports = np.arange(1024, 1024 + WORD0_PORTS)
    one = np.ones((WORD0_PORTS, 1), dtype=np.uint8)
    return _grid_totals(side_hash(one * np.array(WORD0_SRC[s], dtype=np.uint8), ports), side_hash(one * np.array(WORD0_DST[d], dtype=np.uint8), ports))


def _word0_key(t):
    return ((t >> np.uint64(32)) << np.uint64(10)) | vhome(t, 1024).astype(np.uint64)


def search_word0(n_pairs=48, passes=4):
    """Over 2^25 tuples in 32 chunks of 2^20. Memory stays modest: per pass only the keys (upper word, home) of a quarter of the
    homes are kept and sorted; a last pass finds the tuples that carry the keys seen twice."""
    chunks = [(s, d) for s in range(len(WORD0_SRC)) for d in range(len(WORD0_DST))]
    twice = []
    for part in range(passes):
        keys = []
        for s, d in chunks:
            key = _word0_key(_word0_chunk(s, d))
            keys.append(key[(key & np.uint64(1023)) % np.uint64(passes) == np.uint64(part)])
        keys = np.sort(np.concatenate(keys))
        twice.append(np.unique(keys[1:][keys[1:] == keys[:-1]]))
    twice = np.concatenate(twice)
    found = {}
    for s, d in chunks:
        t = _word0_chunk(s, d)
        key = _word0_key(t)
        for ix in np.flatnonzero(np.isin(key, twice)):
            found.setdefault(int(key[ix]), []).append(dict(
                src="%d.%d.%d.%d" % WORD0_SRC[s], sport=1024 + int(ix) // WORD0_PORTS, dst="%d.%d.%d.%d" % WORD0_DST[d], dport=1024 + int(ix) % WORD0_PORTS,
                proto=6, total="%x" % int(t[ix]), home=int(key[ix]) & 1023))
    pairs = [v[:2] for _, v in sorted(found.items()) if len(v) >= 2 and v[0]["total"] != v[1]["total"]]
    return dict(searched=len(chunks) * WORD0_PORTS * WORD0_PORTS, candidates=len(pairs), pairs=pairs[:n_pairs])
