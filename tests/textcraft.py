"""A battery of records whose VALUES are enumerated, for the line encoders' text helpers (csrc/nfagg_flp_line.h ip_text, dec<3|5|10|20>,
dec_i64, mac_text; nfagg_encode.h flow_time; nfagg_conn_meta.h hex_u64). numpy only, no import of the product: the record dtypes are handed
in. The seeded streams of the line tests reach these shapes by luck (tests/test_textcraft_cpu.py counts what they reach); here each is
planted, in four families:

  addr     all 256 zero / non-zero patterns of the eight groups of an IPv6 address in three width classes of the non-zero groups (one hex
           digit, four, mixed 1..4), pattern p in src_ip and partner(p) in dst_ip of the same record; v4-mapped addresses with every octet
           from {0, 9, 10, 99, 100, 255}; the near-misses of the v4 test. The xlat part carries patterns too.
  digits   record j sets every numeric field to the j-th edge of the field's width (EDGES), signed parts to theirs (LATENCY, RTT, RET), the
           TLS ids to the ones without a name (TLS_FALLBACK_IDS), the MAC bytes to MAC_BYTES; protocols cycle so that ports, Flags and Icmp*
           are live.
  clocks   per call (CLOCKS: now, mono, TimeReceived) the time stamps of clock_cases(): both carries of time.Time.Add, millisecond
           boundaries, the epoch, ts = 0 and 2^64 - 1, delta = 2^63.
  hash_id  tracked flows with one conntrack id per hex width (HASH_IDS).

battery() returns them as one Battery; arrange() lays a battery out for the waves of the kernels: interleaved, grouped, odd lane."""
from collections import namedtuple

import numpy as np

M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
V4MAP = bytes(10) + b"\xff\xff"
FEAT = {"additional": 1, "dns": 2, "drops": 4, "network_events": 8, "xlat": 16, "quic": 32}      # NFAGG_FEAT_*
KINDS = ("additional", "dns", "drops", "xlat", "quic")
WIDTH_CLASSES = ("one", "four", "mixed")
MIXED = (0x10, 0x100, 0x1000, 0xf, 0xff, 0xfff, 0x1, 0xabcd)
OCTETS = (0, 9, 10, 99, 100, 255)

Battery = namedtuple("Battery", "recs present parts ids family")

# ---- the edges of a decimal field, by the digits its type can have. The values behind the strconv edges are the varint edges 2^(7k) - 1 and
# 2^(7k) the type reaches: the protobuf encoder sees every varint length of every field.
_D3 = [0, 9, 10, 99, 100, 255]
_D5 = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535]
_D10 = [v for k in range(1, 10) for v in (10**k - 1, 10**k)] + [2**32 - 1]
_D20 = [v for k in range(1, 20) for v in (10**k - 1, 10**k)] + [2**63, 2**64 - 1, 10**9 + 1, 10**18 + 1, 999999999 * 10**9, 10**18 + 10**9]
DECIMAL_EDGES = {3: _D3, 5: _D5, 10: _D10, 20: _D20}                  # the strconv edges alone


def _varints(bits):
    return [v for k in range(1, 10) for v in (2**(7 * k) - 1, 2**(7 * k)) if v < 2**bits]


EDGES = {3: _D3 + _varints(8), 5: _D5 + _varints(16), 10: _D10 + _varints(32), 20: _D20 + _varints(64)}
# DnsLatencyMs = Duration(latency).Milliseconds(): truncation towards zero, both signs; as the uint64 the part holds
LATENCY = [0] + [v & M64 for x in [1, 999_999, 10**6] + [10**k * 10**6 for k in range(1, 13)] for v in (x, -x)] + [2**63, 2**64 - 1]
RTT = [1] + [v for k in range(1, 19) for v in (10**k - 1, 10**k)] + [2**63 - 1, 2**63, 2**64 - 1]
RET = [v for x in [1] + [10**k for k in range(1, 10)] for v in (x, -x)] + [-2**31, 2**31 - 1]
TLS_FALLBACK_IDS = [0x000A, 0x00A0, 0x0A00, 0xA000, 0xFFFF]          # "0x%04X": each hex digit position, a letter in each
HASH_IDS = [0] + [v for w in range(1, 17) for v in (16**(w - 1), 16**w - 1)]      # "%x" of every width, smallest and largest
DROP_CAUSES = [2, 5, (3 << 16) + 1, (1 << 24) + 3]
# mac_text: 0, 9, a and f in either nibble, around the step from digits to letters
MAC_BYTES = [0x00, 0x09, 0x0a, 0x0f, 0x10, 0x90, 0x99, 0x9a, 0xa0, 0xa9, 0xaf, 0xf0, 0xf9, 0xfa, 0xff, 0x5c]
# json key -> the width of its dec<>, for the keys whose value is the number itself. A gated key (absent when its field is 0) has no edge 0.
FIELD_WIDTH = {"Bytes": 20, "Packets": 10, "Sampling": 10, "SrcPort": 5, "DstPort": 5, "Etype": 5, "Flags": 5, "DnsFlags": 5, "DnsId": 5,
               "PktDropBytes": 5, "PktDropPackets": 5, "PktDropLatestFlags": 5, "XlatSrcPort": 5, "XlatDstPort": 5, "ZoneId": 5, "Dscp": 3,
               "Proto": 3, "IcmpType": 3, "IcmpCode": 3, "DnsErrno": 3, "QuicSeenLongHdr": 3, "QuicSeenShortHdr": 3}
GATED = ("Bytes", "Packets", "Sampling", "DnsId", "DnsErrno", "XlatSrcPort", "XlatDstPort")

# ---- the calls: (now_sec, now_nsec, mono, TimeReceived). now = now_sec * 10^9 + now_nsec with 0 <= now_nsec < 10^9, as time.Unix(0, now) holds it.
CLOCKS = [(1_700_000_000, 0, 2_500_000, 0), (1_700_000_000, 999_999_999, 10**15 + 7, -1), (0, 1, 0, I64_MIN), (0, 500_000_000, 2**63, I64_MAX),
          (-2, 1, 2**64 - 1, 1_700_000_003), (-1_000_000, 999_999_999, 123_456_789, 0), (0, 0, 5, -1)]


def now_of(clock):
    return clock[0] * 10**9 + clock[1]


def wrap_i64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


# ---- addresses
def zero_runs(p):
    """[(start, length)] of the runs of zero groups of pattern p (bit k set: group k is not zero), runs of two or more only."""
    runs, k = [], 0
    while k < 8:
        j = k
        while j < 8 and not (p >> j) & 1:
            j += 1
        if j - k >= 2:
            runs.append((k, j - k))
        k = max(j, k + 1)
    return runs


def tie_patterns():
    """The patterns in which the longest run of zero groups occurs twice or more: "the first one" is a decision."""
    out = []
    for p in range(256):
        lens = [n for _, n in zero_runs(p)]
        if lens and lens.count(max(lens)) >= 2:
            out.append(p)
    return out


def partner(p):
    """The pattern on the other side of a record: 5 p + 1 mod 256. A bijection, and never p itself (4 p + 1 is odd); the complement
    rotated by r groups keeps 0x55 (r = 1, 3) or 0x33 (r = 2) in place."""
    return (5 * p + 1) & 255


def xlat_partner(p):
    """Rotation by three groups: a bijection that keeps 0 with 0 (an all-zero address on either side removes both Xlat keys)."""
    return ((p << 3) | (p >> 5)) & 255


def group_value(cls, p, k):
    if cls == "one":
        return 1 + (k + p) % 15
    if cls == "four":
        return 0x1000 + (k * 0x1357 + p * 0x0321) % 0xEFFF            # 0x1000 .. 0xfffe: group 5 never completes a v4-mapped prefix
    return MIXED[(k + p) % len(MIXED)]


def addr_of(p, cls):
    """The 16 bytes of pattern p in width class cls."""
    out = bytearray(16)
    for k in range(8):
        if (p >> k) & 1:
            v = group_value(cls, p, k)
            out[2 * k], out[2 * k + 1] = v >> 8, v & 255
    return bytes(out)


def pattern_of(b):
    return sum(1 << k for k in range(8) if b[2 * k] or b[2 * k + 1])


def near_misses():
    """[(src 16 bytes, dst 16 bytes, ethertype)]: addresses one step away from what To4() accepts, and families that disagree with the
    ethertype."""
    tail = bytes([10, 0, 9, 255])
    out = [(bytes(10) + b"\xff\xfe" + tail, bytes(10) + b"\xfe\xff" + tail, 0x86DD)]
    for k in (0, 5, 9):
        a = bytearray(V4MAP + tail)
        a[k] = 1 + k
        b = bytearray(V4MAP + bytes(4))
        b[9 - k] = 0x80
        out.append((bytes(a), bytes(b), 0x86DD if k else 0x0800))
    out.append((V4MAP + bytes(4), V4MAP + tail, 0x86DD))               # ::ffff:0:0 and a mapped address under the IPv6 ethertype
    out.append((addr_of(0b10000001, "mixed"), addr_of(0xff, "four"), 0x0800))      # unmapped addresses under the IPv4 ethertype
    out.append((bytes(16), bytes(15) + b"\x01", 0x0800))
    return out


def _ip(a, i, b):
    a[i] = np.frombuffer(b, dtype=np.uint8)


def base_records(FLOW_RECORD, n, mono):
    """n copies of one plain v4 / TCP record, a millisecond old at a call whose monotonic clock reads mono."""
    r = np.zeros(n, dtype=FLOW_RECORD)
    i, m = r["id"], r["metrics"]
    i["src_ip"] = np.frombuffer(V4MAP + bytes([10, 0, 0, 1]), dtype=np.uint8)
    i["dst_ip"] = np.frombuffer(V4MAP + bytes([10, 0, 1, 7]), dtype=np.uint8)
    i["src_port"], i["dst_port"], i["transport_protocol"] = 40000, 443, 6
    m["eth_protocol"], m["bytes"], m["packets"], m["flags"], m["if_index_first_seen"] = 0x0800, 1500, 3, 0x12, 2
    m["start_mono_time_ts"] = np.uint64((mono - 2_000_000) & M64)
    m["end_mono_time_ts"] = np.uint64((mono - 1_000_000) & M64)
    m["src_mac"] = np.frombuffer(bytes.fromhex("0a1b2c3d4e5f"), dtype=np.uint8)
    m["dst_mac"] = np.frombuffer(bytes.fromhex("f0e1d2c3b4a5"), dtype=np.uint8)
    return r


def empty_parts(PART_DTYPES, n):
    return {k: np.zeros(n, dtype=PART_DTYPES[k]) for k in KINDS}


def addr_family(FLOW_RECORD, PART_DTYPES, mono):
    pats = [(p, cls) for cls in WIDTH_CLASSES for p in range(256)]
    misses = near_misses()
    n = len(pats) + 2 * len(OCTETS) + len(misses)
    r, present, parts = base_records(FLOW_RECORD, n, mono), np.zeros(n, dtype=np.uint8), empty_parts(PART_DTYPES, n)
    i, m, x = r["id"], r["metrics"], parts["xlat"]
    i["transport_protocol"] = np.array([6, 17, 132, 1, 58], dtype=np.uint8)[np.arange(n) % 5]
    for j, (p, cls) in enumerate(pats):
        _ip(i["src_ip"], j, addr_of(p, cls))
        _ip(i["dst_ip"], j, addr_of(partner(p), cls))
        m["eth_protocol"][j] = 0x86DD
        q = (p + 85) & 255                                           # the xlat pair of the record: other patterns than its own two
        _ip(x["saddr"], j, addr_of(q, cls))
        _ip(x["daddr"], j, addr_of(xlat_partner(q), cls))
        x["sport"][j], x["dport"][j], x["zone_id"][j] = p, 256 + p, j
        present[j] = FEAT["xlat"]
    j = len(pats)
    for k in range(2 * len(OCTETS)):                                 # every octet position takes every value, on both sides
        _ip(i["src_ip"], j, V4MAP + bytes(OCTETS[(k + o) % 6] for o in range(4)))
        _ip(i["dst_ip"], j, V4MAP + bytes(OCTETS[(k + 2 * o + 1) % 6] for o in range(4)))
        _ip(x["saddr"], j, V4MAP + bytes(OCTETS[(k + 3 * o + 2) % 6] for o in range(4)))
        _ip(x["daddr"], j, V4MAP + bytes(OCTETS[(k + 5 * o + 3) % 6] for o in range(4)))     # none of the four is 0.0.0.0 for any k
        present[j] = FEAT["xlat"]
        j += 1
    for s, d, eth in misses:
        _ip(i["src_ip"], j, s)
        _ip(i["dst_ip"], j, d)
        _ip(x["saddr"], j, d)
        _ip(x["daddr"], j, s)
        m["eth_protocol"][j] = eth
        present[j] = FEAT["xlat"]
        j += 1
    assert j == n
    return r, present, parts


def digits_family(FLOW_RECORD, PART_DTYPES, mono):
    """Block A (len(EDGES[20]) records): IP records whose protocol cycles 6, 17, 1, 58, 132, 6; block B: Proto takes its own edges; block C:
    Etype takes its own, most of them not IP. Every other field goes on cycling through its list in all three."""
    e3, e5, e10, e20 = EDGES[3], EDGES[5], EDGES[10], EDGES[20]
    na, nb, nc = len(e20), len(e3), len(e5)
    n = na + nb + nc
    r, parts = base_records(FLOW_RECORD, n, mono), empty_parts(PART_DTYPES, n)
    present = np.full(n, sum(FEAT[k] for k in KINDS), dtype=np.uint8)
    j = np.arange(n)
    pick = lambda xs, shift=0, dtype=np.uint64: np.array(xs, dtype=dtype)[(j + shift) % len(xs)]  # noqa: E731
    nz = lambda xs: [v for v in xs if v]  # noqa: E731
    i, m = r["id"], r["metrics"]
    i["transport_protocol"] = pick([6, 17, 1, 58, 132, 6])
    i["transport_protocol"][na:na + nb] = e3
    m["eth_protocol"] = np.where(j % 2 == 0, 0x0800, 0x86DD)
    m["eth_protocol"][na + nb:] = e5
    for k in range(n):
        if m["eth_protocol"][k] == 0x86DD:
            _ip(i["src_ip"], k, addr_of(0b10000001, "mixed"))
            _ip(i["dst_ip"], k, addr_of(0b11000011, "one"))
    i["src_port"], i["dst_port"], i["icmp_type"], i["icmp_code"] = pick(e5), pick(e5, 3), pick(e3), pick(e3, 3)
    m["bytes"], m["packets"], m["sampling"], m["flags"], m["dscp"] = pick(e20), pick(e10), pick(e10, 5), pick(e5, 6), pick(e3, 5)
    m["direction_first_seen"], m["nb_observed_intf"] = pick(e3, 1), 6
    for k in range(6):
        m["observed_direction"][:, k] = pick(e3, k + 2)
        m["observed_intf"][:, k] = 3 + k
        m["src_mac"][:, k], m["dst_mac"][:, k] = pick(MAC_BYTES, k), pick(MAC_BYTES, 7 + 3 * k)
    m["ssl_version"], m["tls_cipher_suite"], m["tls_key_share"] = pick(TLS_FALLBACK_IDS), pick(TLS_FALLBACK_IDS, 1), pick(e5, 9)
    m["misc_flags"], m["tls_types"] = j & 1, pick([0, 1, 63, 0x40])
    a, d, p, x, q = (parts[k] for k in KINDS)
    a["flow_rtt"], a["ipsec_encrypted_ret"], a["ipsec_encrypted"] = pick(RTT), pick(RET, dtype=np.int64), j % 3
    d["id"], d["flags"], d["errno_"], d["latency"] = pick(nz(e5)), pick(e5, 2), pick(nz(e3)), pick(LATENCY)
    name = b"\x03www\x07example\x03com"
    d["name"][:, :len(name)] = np.frombuffer(name, dtype=np.uint8)
    p["bytes"], p["packets"], p["latest_flags"], p["latest_drop_cause"], p["latest_state"] = pick(e5, 4), pick(e5, 7), pick(e5, 1), pick(DROP_CAUSES), j % 13
    x["saddr"] = np.frombuffer(V4MAP + bytes([10, 9, 0, 100]), dtype=np.uint8)
    x["daddr"] = np.frombuffer(addr_of(0b00100101, "mixed"), dtype=np.uint8)
    x["sport"], x["dport"], x["zone_id"] = pick(e5, 8), pick(e5, 11), pick(e5, 5)
    q["version"], q["seen_long_hdr"], q["seen_short_hdr"] = pick(e10, 2), pick(e3, 4), pick(e3, 7)
    return r, present, parts


def clock_cases(clock):
    """[(name, ts)]: the time stamps of one call. d = ts - mono, wrapped to int64, is what flow_time adds to now."""
    now_sec, nsec, mono, _ = clock
    now, G = now_of(clock), 10**9
    d = {"delta 0": 0, "delta +1": 1, "delta -1": -1, "nsec sum 10^9 - 1": 3 * G + (G - 1 - nsec), "nsec sum 0": -2 * G - nsec,
         "time nsec 999999": 7 * G + 999_999 - nsec, "time nsec 1000000": -5 * G + 1_000_000 - nsec,
         "wall -1 ns": -now - 1, "wall 0": -now, "wall +1 ns": -now + 1, "delta 2^63": I64_MIN}
    if nsec >= 1:
        d["nsec sum 10^9"] = 4 * G + (G - nsec)                     # no remainder of d reaches 10^9 from 0
    if nsec <= G - 2:
        d["nsec sum -1"] = -6 * G - nsec - 1
    out = [(name, (mono + v) & M64) for name, v in d.items()]
    return out + [("ts 0", 0), ("ts 2^64 - 1", M64)]


def clocks_family(FLOW_RECORD, PART_DTYPES, clock):
    cases = clock_cases(clock)
    n = len(cases)
    r = base_records(FLOW_RECORD, n, clock[2])
    ts = np.array([t for _, t in cases], dtype=np.uint64)
    r["metrics"]["start_mono_time_ts"], r["metrics"]["end_mono_time_ts"] = ts, np.roll(ts, -5)
    r["id"]["transport_protocol"] = np.array([6, 17, 1], dtype=np.uint8)[np.arange(n) % 3]
    return r, np.zeros(n, dtype=np.uint8), empty_parts(PART_DTYPES, n)


def hash_family(FLOW_RECORD, PART_DTYPES, mono):
    n = len(HASH_IDS)
    r = base_records(FLOW_RECORD, n, mono)
    r["id"]["transport_protocol"] = np.array([6, 17, 132], dtype=np.uint8)[np.arange(n) % 3]
    r["id"]["src_port"] = 1024 + np.arange(n)
    for k in range(1, n, 4):
        r["metrics"]["eth_protocol"][k] = 0x86DD
        _ip(r["id"]["src_ip"], k, addr_of(0b10000011, "mixed"))
        _ip(r["id"]["dst_ip"], k, addr_of(0b10000000, "one"))        # ::<digit>
    return r, np.zeros(n, dtype=np.uint8), empty_parts(PART_DTYPES, n)


def _fmix(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    return x ^ (x >> 33)


def concat(batteries):
    return Battery(np.concatenate([b.recs for b in batteries]), np.concatenate([b.present for b in batteries]),
                   {k: np.concatenate([b.parts[k] for b in batteries]) for k in KINDS}, np.concatenate([b.ids for b in batteries]),
                   np.concatenate([b.family for b in batteries]))


def take(b, idx):
    idx = np.asarray(idx, dtype=np.int64)
    return Battery(b.recs[idx].copy(), b.present[idx].copy(), {k: v[idx].copy() for k, v in b.parts.items()}, b.ids[idx].copy(), b.family[idx].copy())


def family(FLOW_RECORD, PART_DTYPES, name, clock=CLOCKS[0]):
    """One family as a Battery. The conntrack ids of the families other than hash_id are a fixed scramble of the index."""
    make = {"addr": addr_family, "digits": digits_family, "hash_id": hash_family}
    r, present, parts = clocks_family(FLOW_RECORD, PART_DTYPES, clock) if name == "clocks" else make[name](FLOW_RECORD, PART_DTYPES, clock[2])
    ids = np.array(HASH_IDS if name == "hash_id" else [_fmix(k + 1) >> (k % 61) for k in range(len(r))], dtype=np.uint64)
    return Battery(r, present, parts, ids, np.full(len(r), name, dtype="U8"))


FAMILIES = ("addr", "digits", "clocks", "hash_id")


def battery(FLOW_RECORD, PART_DTYPES, clock=CLOCKS[0]):
    """The four families behind one another, for the call `clock`."""
    return concat([family(FLOW_RECORD, PART_DTYPES, f, clock) for f in FAMILIES])


def plain(FLOW_RECORD, PART_DTYPES, n, clock=CLOCKS[0]):
    r = base_records(FLOW_RECORD, n, clock[2])
    return Battery(r, np.zeros(n, dtype=np.uint8), empty_parts(PART_DTYPES, n), np.full(n, 0x1234abcd, dtype=np.uint64), np.full(n, "plain", dtype="U8"))


def without_tls(recs):
    """The records with their TLS fields cleared: what the entry points that defer such records can take."""
    r = recs.copy()
    for f in ("ssl_version", "tls_cipher_suite", "tls_key_share"):
        r["metrics"][f] = 0
    return r


def coverage(recs):
    """What a set of records reaches of the value shapes, counted on the records alone: the zero / non-zero patterns and the tie patterns
    among the IPv6 texts of src_ip and dst_ip (IP ethertype, not v4-mapped), and the strconv edges 10^k - 1 / 10^k (k >= 1) of Bytes, Packets,
    Sampling and the two ports."""
    m, i = recs["metrics"], recs["id"]
    ip = np.isin(m["eth_protocol"], (0x0800, 0x86DD))
    pats = set()
    for side in ("src_ip", "dst_ip"):
        a = i[side][ip]
        v6 = ~((a[:, :10] == 0).all(axis=1) & (a[:, 10] == 0xFF) & (a[:, 11] == 0xFF))
        g = (a[v6, 0::2] != 0) | (a[v6, 1::2] != 0)
        pats |= set(np.unique((g * (1 << np.arange(8))).sum(axis=1)).tolist())
    want = {"Bytes": DECIMAL_EDGES[20][:38], "Packets": DECIMAL_EDGES[10][:18], "Sampling": DECIMAL_EDGES[10][:18], "ports": DECIMAL_EDGES[5][1:9]}
    have = {"Bytes": set(m["bytes"].tolist()), "Packets": set(m["packets"].tolist()), "Sampling": set(m["sampling"].tolist()),
            "ports": set(i["src_port"].tolist()) | set(i["dst_port"].tolist())}
    return {"patterns": len(pats), "ties": len(pats & set(tie_patterns())), "edges": sum(len(have[k] & set(want[k])) for k in want),
            "edges_of": sum(len(v) for v in want.values())}


ARRANGEMENTS = ("interleaved", "grouped", "odd lane")
ODD_LANES = (0, 31, 32, 63)
ODD_WAVES = 62


def odd_lane_choice(b):
    """The battery records that stand alone in a wave of plain ones: one address per tie pattern (the width class cycling), every third
    digits record, every second clocks record, every fifth id; ODD_WAVES of them."""
    fam = b.family
    addr = np.flatnonzero(fam == "addr")
    ties = [addr[256 * (k % 3) + p] for k, p in enumerate(tie_patterns())]
    rest = np.concatenate([np.flatnonzero(fam == "digits")[::3], np.flatnonzero(fam == "clocks")[::2], np.flatnonzero(fam == "hash_id")[::5]])
    return np.concatenate([ties, rest]).astype(np.int64)[:ODD_WAVES]


def arrange(b, how, FLOW_RECORD, PART_DTYPES, clock=CLOCKS[0]):
    """interleaved: a fixed permutation (a stride coprime to the length, near the golden section), so that neighbouring lanes hold different
    families and values. grouped: whole waves of one family, a family's last wave filled up with its first records. odd lane: waves of 63
    plain records and one battery record at lane 0, 31, 32 or 63."""
    n = len(b.recs)
    if how == "interleaved":
        stride = next(s for s in range(int(n * 0.618), n) if np.gcd(s, n) == 1)
        return take(b, (np.arange(n) * stride) % n)
    if how == "grouped":
        idx = []
        for f in FAMILIES:
            own = np.flatnonzero(b.family == f)
            idx.append(own[np.arange(-(-len(own) // 64) * 64) % len(own)])
        return take(b, np.concatenate(idx))
    assert how == "odd lane"
    chosen = odd_lane_choice(b)
    out = plain(FLOW_RECORD, PART_DTYPES, 64 * len(chosen), clock)
    for w, k in enumerate(chosen):
        at = 64 * w + ODD_LANES[w % 4]
        out.recs[at], out.present[at], out.ids[at], out.family[at] = b.recs[k], b.present[k], b.ids[k], b.family[k]
        for kind in KINDS:
            out.parts[kind][at] = b.parts[kind][k]
    return out
