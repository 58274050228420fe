"""Network-event inputs built on purpose (a helper module, no fixtures; numpy only, no import of the product: the record dtypes are
handed in and written through their bytes, bpf/types.h:153-161 and the 32-byte pkt_drop_metrics). Four families for
csrc/nfagg_netev.hip and the *_netev encoders:

    scripts   every sequence of four slot symbols over Z M U A1 A2 D1 D2 D3 T T2 (10^4 scripts), under four states of the flow's
              drops part, against two tables that hold the same ten rows: alone (searched in LDS) and among 300-odd filler rows
              (searched in HBM). record.go:126-157 reads, per slot, packets == 0, the decoder's answer, String(), the drop cause:
              the symbols are the classes of that, twice where an order can matter (two rows of one String(), two drop causes).
    search    cookies that differ in one dword, in bit 63, in bit 0, by a byte swap; the ends of the 64-bit range; tables of evenly
              spaced cookies at the row counts where the search turns (1, 2, 3, around the LDS threshold, around 1024, the
              format's maximum, whose last row 0xFFFE sits next to NO_ROW).
    missing   cookies with a chosen home slot in the missing-cookie set, through the inverse of splitmix64's finalizer: one home,
              chains through slot 0, sets filled exactly and one over, the all-zero cookie beside a full set.
    pieces    Message events of every text length 0..140 and 484..498: every residue of the rendered length mod 16, the protobuf
              lengths across 127 / 128, both renderings at the 512-byte cap.

Answers are netev_ref's: {cookie (8 bytes): ACL tuple | bytes | None}."""
from types import SimpleNamespace

import numpy as np

FEAT_DROPS, FEAT_NETEV = 4, 8
NO_ROW = 0xFFFF
MAX_ROWS = 65535
M64 = (1 << 64) - 1
LDS_ROWS = 256                                             # kNetevLdsRows


def ck(v: int) -> bytes:
    return int(v).to_bytes(8, "little")


def _fill(n, netev_dtype, drops_dtype, rng):
    """n flows of random bytes: (netev bytes [n, 72], drops bytes [n, 32])."""
    assert np.dtype(netev_dtype).itemsize == 72 and np.dtype(drops_dtype).itemsize == 32
    return rng.integers(0, 256, (n, 72), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _put_slots(ne, cookies, by, pk):
    """cookies uint64[n, 4], bytes / packets [n, 4] into the network-events bytes (cookies@16, bytes@48, packets@56)."""
    n = len(ne)
    ne[:, 16:48] = np.ascontiguousarray(cookies, dtype="<u8").view(np.uint8).reshape(n, 32)
    ne[:, 48:56] = np.ascontiguousarray(by, dtype="<u2").view(np.uint8).reshape(n, 8)
    ne[:, 56:64] = np.ascontiguousarray(pk, dtype="<u2").view(np.uint8).reshape(n, 8)


# ---------------------------------------------------------------- scripts
SYMBOLS = ("Z", "M", "U", "A1", "A2", "D1", "D2", "D3", "T", "T2")
S1 = "Allowed by network policy p in namespace ns, direction Ingress"
S2 = "Dropped by network policy p in namespace ns, direction Ingress"
S3 = "sampled by something that is no ACL"
# Sorted, the S1 class is A2 < D3 < A1 and the S2 class T2 < D2 < D1: the first row of a class is neither the plain allow nor the
# known-actor drop. T is the table's first row (class number 0, what an unset `seen` entry holds). A1 and A2 share their low dword,
# A2 and D3 their high one; A1 and D1 have bit 63. M has no row: T2 has its low dword, the decoy X its high dword and the next value.
COOKIE = {"T": 0x00000000FFFFFFFF, "A2": 0x0000000100000005, "D3": 0x0000000180000005, "T2": 0x0000000200000007, "M": 0x0000000300000007,
          "X": 0x0000000300000008, "U": 0x4000000000000000, "D2": 0x7FFFFFFFFFFFFFFF, "A1": 0x8000000000000005, "D1": 0x8000000000000006,
          "Z": 0xFFFFFFFFFFFFFFFE}
EVENT = {
    "Z": ("drop", "UDNIsolation", "", "", "", "Dropped by UDN isolation of type "),       # only ever met with packets == 0
    "U": None,
    "A1": ("allow", "NetworkPolicy", "p", "ns", "Ingress", S1),
    "A2": ("allow-related", "AdminNetworkPolicy", "q", "ns", "Egress", S1),
    "D1": ("drop", "NetworkPolicy", "p", "ns", "Ingress", S2),                              # cause (1 << 24) + 4
    "D2": ("drop", "NoSuchActor", 'r"\\\n', "", "Egress", S2),                              # cause (1 << 24) + 0
    "D3": ("drop", "EgressFirewall", "fw", "ns", "Egress", S1),                             # cause (1 << 24) + 1
    "T": S3.encode(),
    "T2": S2.encode(),                                                                      # no ACL: injects nothing
    "X": ("drop", "MulticastNS", "m", "ns", "", "the row after the cookie without one"),    # never in a script
}
N_SCRIPTS = 10 ** 4
COUNTS = np.array([1, 0x8000, 0xFFFF, 0x7FFF], dtype=np.uint16)
STATES = ("present bit clear", "present, small counts", "present, 0xFFFE / 0xFFFF", "drops array NULL")
SMALL = dict(bytes=1, packets=1, cause=7, flags=0x12, state=3)


def script_symbols(script):
    """The four symbol numbers of every script: its decimal digits, slot 0 first."""
    s = np.asarray(script)
    return np.stack([(s // 10 ** (3 - k)) % 10 for k in range(4)], axis=-1)


def describe(script: int, state: int) -> str:
    return "script %s, drops state: %s" % (" ".join(SYMBOLS[k] for k in script_symbols(script)), STATES[state])


def small_answers() -> dict:
    return {ck(COOKIE[s]): EVENT[s] for s in EVENT}


def big_answers(seed=1) -> dict:
    """The ten rows among fillers: 300 cookies drawn above T's, both second neighbours of every answer and the value before M."""
    rng = np.random.default_rng(seed)
    taken = set(COOKIE.values())
    fill = [int(v) for v in rng.integers(1 << 32, M64, 300, dtype=np.uint64)]
    fill += [(c + d) & M64 for c in COOKIE.values() for d in (-2, 2)] + [COOKIE["M"] - 1]
    out = small_answers()
    for k, c in enumerate(dict.fromkeys(c for c in fill if c not in taken and c > COOKIE["T"])):
        out[ck(c)] = None if k % 3 == 0 else b"filler %d" % k if k % 3 == 1 else ("allow", "NetpolNode", "f%d" % k, "", "Ingress", "filler acl %d" % k)
    return out


def script_call(netev_dtype, drops_dtype, states, seed=2):
    """All 10^4 scripts once per state, and after every script with script % 7 == 3 a copy whose NFAGG_FEAT_NETWORK_EVENTS bit is
    clear (one flow in eight). states (3,) is the call without a drops array. Returns present, netev, drops (None for state 3),
    script, state, live."""
    rng = np.random.default_rng(seed + 10 * sum(states))
    s = np.arange(N_SCRIPTS)
    script1 = np.repeat(s, 1 + (s % 7 == 3))
    live1 = np.r_[True, script1[1:] != script1[:-1]]
    script, live, state = np.tile(script1, len(states)), np.tile(live1, len(states)), np.repeat(np.array(states), len(script1))
    n = len(script)
    ne, dr = _fill(n, netev_dtype, drops_dtype, rng)
    sym = script_symbols(script)
    at = (script[:, None] + np.arange(4)) % 4
    pk = COUNTS[3 - at]
    pk[sym == SYMBOLS.index("Z")] = 0
    _put_slots(ne, np.array([COOKIE[k] for k in SYMBOLS], dtype=np.uint64)[sym], COUNTS[at], pk)
    present = (rng.integers(0, 256, n, dtype=np.uint8) & 0x33) | np.where(live, FEAT_NETEV, 0).astype(np.uint8)
    present[(state == 1) | (state == 2)] |= FEAT_DROPS
    present[state == 3] |= rng.integers(0, 2, int((state == 3).sum()), dtype=np.uint8) * FEAT_DROPS     # no array: the bit says nothing
    d = dr.view(drops_dtype).reshape(n)                                    # bytes@16 packets@18 cause@20 flags@24 state@28, pad@29
    f16, f32 = dr.view("<u2"), dr.view("<u4")
    m = state == 1
    f16[m, 8], f16[m, 9], f32[m, 5], f16[m, 12], dr[m, 28] = SMALL["bytes"], SMALL["packets"], SMALL["cause"], SMALL["flags"], SMALL["state"]
    m = state == 2
    f16[m, 8], f16[m, 9] = 0xFFFE, 0xFFFF
    return SimpleNamespace(present=present, netev=ne.view(netev_dtype).reshape(n), drops=None if states == (3,) else d, script=script, state=state,
                           live=live, n=n)


# ---------------------------------------------------------------- search
EDGES = (0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, M64 - 1, M64)
SIZES = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, MAX_ROWS)


def bswap(x: int) -> int:
    return int.from_bytes(ck(x), "big")


def search_cookies(seed=3):
    """The crafted table's cookies: the edges, x / x ^ 2^32 / x ^ 1 and x / byte-swapped x for three random x each."""
    rng = np.random.default_rng(seed)
    xs = [int(v) for v in rng.integers(1 << 40, M64 - (1 << 40), 6, dtype=np.uint64)]
    out = list(EDGES)
    for x in xs[:3]:
        out += [x, x ^ (1 << 32), x ^ 1]
    for x in xs[3:]:
        out += [x, bswap(x)]
    assert len(set(out)) == len(out)
    return out


def search_answers(cookies) -> dict:
    """One decodable row per cookie with a String() of its own: every third a dropping ACL."""
    return {ck(c): ("drop", "EgressFirewall", "n%d" % k, "ns", "Egress", "acl %016x" % c) if k % 3 == 0 else b"cookie %016x" % c
            for k, c in enumerate(cookies)}


def neighbours(cookies):
    """Every cookie +- 1 (mod 2^64) that is no cookie itself, in order, once."""
    have = set(cookies)
    return list(dict.fromkeys(v for c in cookies for v in ((c - 1) & M64, (c + 1) & M64) if v not in have))


def spaced_cookies(rows: int):
    """rows evenly spaced cookies, none of them 0 or 2^64 - 1: there is room below the first and above the last."""
    step = (1 << 64) // (rows + 1)
    return np.arange(1, rows + 1, dtype=np.uint64) * np.uint64(step)


def spaced_answers(rows: int) -> dict:
    """Up to 1 025 rows a String() each; at the maximum one String() for all (the host's class scan stays linear) and the row number in
    the ACL's name, so the rendered pieces still tell the rows apart."""
    cookies = spaced_cookies(rows).tolist()
    if rows <= 1025:
        return {ck(c): b"row %d" % r for r, c in enumerate(cookies)}
    return {ck(c): ("allow", "NetworkPolicy", "n%d" % r, "ns", "Ingress", "shared") for r, c in enumerate(cookies)}


def probe_flows(cookies, netev_dtype, drops_dtype, seed=4):
    """One flow per cookie with ONE live slot (slot i % 4); the other three hold the next cookies of the list with packets == 0.
    Returns (present, netev, drops): no flow has a drops part."""
    c = np.array(cookies, dtype=np.uint64)
    n = len(c)
    ne, dr = _fill(n, netev_dtype, drops_dtype, np.random.default_rng(seed))
    i = np.arange(n)
    slot = (np.arange(4)[None, :] - i[:, None]) % 4                          # 0 at the live slot
    pk = np.where(slot == 0, 1 + i[:, None] % 3, 0)
    _put_slots(ne, c[(i[:, None] + slot) % n], np.where(slot == 0, 40 + i[:, None] % 7, 9), pk)
    return np.full(n, FEAT_NETEV, dtype=np.uint8), ne.view(netev_dtype).reshape(n), dr.view(drops_dtype).reshape(n)


# ---------------------------------------------------------------- missing
CAPS = (1, 2, 3, 7, 64, 100, 1000)
_M1, _M2 = 0xbf58476d1ce4e5b9, 0x94d049bb133111eb
_I1, _I2 = pow(_M1, -1, 1 << 64), pow(_M2, -1, 1 << 64)


def mix(x: int) -> int:
    """splitmix64's finalizer."""
    x ^= x >> 30
    x = (x * _M1) & M64
    x ^= x >> 27
    x = (x * _M2) & M64
    return x ^ (x >> 31)


def _unshift(v: int, s: int) -> int:
    x = v
    for _ in range(64 // s + 1):
        x = v ^ (x >> s)
    return x


def unmix(v: int) -> int:
    x = _unshift(v, 31)
    x = _unshift((x * _I2) & M64, 27)
    return _unshift((x * _I1) & M64, 30)


def cookies_at(homes, cap: int, rng):
    """One cookie per entry of homes with mix(cookie) % cap == home: unmix(home + cap * j), j >= 1 drawn, all distinct, none zero."""
    out, used = [], set()
    for h in homes:
        assert 0 <= h < cap
        while True:
            j = 1 + int(rng.integers(0, 1 << 62)) % ((M64 - h) // cap)
            if (h, j) not in used:
                break
        used.add((h, j))
        out.append(unmix(h + cap * j))
    assert 0 not in out and len(set(out)) == len(out)
    return out


def missing_cases(cap: int, seed=5):
    """[(name, cookies, homes)] for one capacity; a cookie of 0 is the all-zero cookie, which has no home."""
    rng = np.random.default_rng(seed + cap)
    cases = []
    home = (5 * cap // 7) % cap
    for m in dict.fromkeys((cap, cap - 1, cap // 2)):                       # cap in {m, m + 1, 2m}
        if m >= 1:
            cases.append(("one_home %d" % m, [home] * m))
    cases.append(("wrap", [(cap - 2 + k % 2) % cap for k in range(min(cap, 6))]))
    spread = [int(v) for v in rng.integers(0, cap, cap + 1)]
    cases.append(("exact", spread[:cap]))
    cases.append(("exact + 1", spread))
    out = [(name, cookies_at(homes, cap, rng), homes) for name, homes in cases]
    exact = out[-2]
    out.append(("zero beside full", exact[1] + [0], exact[2] + [None]))
    out.append(("zero with room", exact[1][:-1] + [0], exact[2][:-1] + [None]))
    return out


def missing_flows(cookies, netev_dtype, drops_dtype, seed=6):
    """Every cookie alone in one slot of at least 64 flows, neighbouring lanes on different cookies, over at least three workgroups
    of 256 lanes; then once in all four slots of one flow."""
    c = np.array(cookies, dtype=np.uint64)
    m = len(c)
    reps = max(64, -(-768 // m))
    f = np.arange(m * reps)
    slot = (np.arange(4)[None, :] - (f // m)[:, None]) % 4
    cookie4 = np.concatenate([np.where(slot == 0, c[f % m][:, None], np.uint64(0x1234)), np.repeat(c[:, None], 4, axis=1)])
    pk = np.concatenate([(slot == 0).astype(np.uint16), np.ones((m, 4), dtype=np.uint16)])
    n = len(pk)
    ne, dr = _fill(n, netev_dtype, drops_dtype, np.random.default_rng(seed))
    _put_slots(ne, cookie4, pk * 3, pk)
    return np.full(n, FEAT_NETEV, dtype=np.uint8), ne.view(netev_dtype).reshape(n), dr.view(drops_dtype).reshape(n)


def off_path(slots, cap: int):
    """The stored cookies that a probe from mix(cookie) % cap would not find: [(slot, cookie)] with an empty slot between the home
    and the slot (both walked upwards, wrapping)."""
    slots = [int(v) for v in slots]
    bad = []
    for at, v in enumerate(slots):
        if v:
            s = mix(v) % cap
            while s != at and slots[s]:
                s = (s + 1) % cap
            if s != at:
                bad.append((at, v))
    return bad


# ---------------------------------------------------------------- pieces
PIECE_T = tuple(range(0, 141)) + tuple(range(484, 499))
PIECE_FLOWS = 64 * 3 + 5
T_CAP = 498


def piece_event(t: int) -> bytes:
    """A Message of t bytes without a byte that escapes: its JSON object has 14 + t bytes. The last one, t = 498, would render to 513
    protobuf bytes and no table takes it; in its place stands a text of 497 bytes that starts with a quote, 498 once escaped: both of
    its renderings have 512 bytes."""
    if t == T_CAP:
        return b'"' + piece_event(T_CAP - 2)
    return bytes(97 + (t + k) % 26 for k in range(t))


def piece_cookie(t: int) -> bytes:
    return ck(0x5000 + t)


def piece_answers() -> dict:
    return {piece_cookie(t): piece_event(t) for t in PIECE_T}


def piece_pb_len(t: int) -> int:
    """0x0A len {0x0A 7 "Message" 0x12 len text}, the text's raw length."""
    raw = len(piece_event(t))
    entry = 9 + 1 + (1 if raw < 128 else 2) + raw
    return 1 + (1 if entry < 128 else 2) + entry


def piece_flows(netev_dtype, drops_dtype, seed=7):
    """Flow i carries the events i, i + 1, i + 2, i + 3 of PIECE_T, cyclically. Returns (present, netev, drops, picks [n, 4])."""
    n = PIECE_FLOWS
    ne, dr = _fill(n, netev_dtype, drops_dtype, np.random.default_rng(seed))
    pick = (np.arange(n)[:, None] + np.arange(4)) % len(PIECE_T)
    _put_slots(ne, np.array([0x5000 + t for t in PIECE_T], dtype=np.uint64)[pick], np.full((n, 4), 2), np.ones((n, 4)))
    return np.full(n, FEAT_NETEV, dtype=np.uint8), ne.view(netev_dtype).reshape(n), dr.view(drops_dtype).reshape(n), pick
