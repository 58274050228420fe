"""tests/textcraft.py held against what it promises, and a second opinion on the restatements the crafted-text GPU tests take their
expected bytes from: every pattern, width class, tie, edge and clock case is in the battery (looked for in the restatement's own lines,
so a gate that hides a value shows); flp_json_ref.go_ip against `ipaddress`, the printed decimals against the records' integers,
unix_milli against floor division in Python integers, DnsLatencyMs against exact truncation; the arrangements' sizes and lanes."""
import fractions
import ipaddress
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_ref as R  # noqa: E402
import flp_json_tls_ref as T  # noqa: E402
import textcraft as tc  # noqa: E402

NAMES = [(2, None, b"eth0", b"default")]
AGENT = bytes(10) + b"\xff\xff" + bytes([10, 1, 2, 3])


@pytest.fixture(scope="module")
def dt(nf):
    return nf.FLOW_RECORD, nf.ROLLUP_KINDS


@pytest.fixture(scope="module")
def bat(dt):
    return tc.battery(*dt)


def lines_of(b, clock, tls_names):
    """The restatement's lines with every key a policy can add: TLS names and the content parts."""
    buf, off = T.encode(b.recs, tls_names, tc.now_of(clock), clock[2], NAMES, AGENT, clock[3], present=b.present, parts=b.parts)
    return buf.split(b"\n")[:-1]


def test_part_bits_are_the_products(nf):
    assert tc.FEAT == {"additional": nf.FEAT_ADDITIONAL, "dns": nf.FEAT_DNS, "drops": nf.FEAT_DROPS, "network_events": nf.FEAT_NETWORK_EVENTS,
                       "xlat": nf.FEAT_XLAT, "quic": nf.FEAT_QUIC}


def test_addr_of_builds_the_pattern_in_its_width_class():
    seen = set()
    for p in range(256):
        for cls in tc.WIDTH_CLASSES:
            a = tc.addr_of(p, cls)
            g = [(a[2 * k] << 8) | a[2 * k + 1] for k in range(8)]
            assert [1 if v else 0 for v in g] == [(p >> k) & 1 for k in range(8)] and tc.pattern_of(a) == p
            nz = [v for v in g if v]
            assert all(v != 0xffff for v in nz)
            if cls == "one":
                assert all(v < 0x10 for v in nz)
            elif cls == "four":
                assert all(v >= 0x1000 for v in nz)
            else:
                seen |= set(nz)
    assert {0x10, 0x100, 0x1000, 0xf, 0xff, 0xfff} <= seen


def test_all_patterns_and_width_classes_on_both_sides_and_in_the_xlat_part(bat):
    want = {tc.addr_of(p, cls) for p in range(256) for cls in tc.WIDTH_CLASSES}
    addr = bat.family == "addr"
    v6 = addr & (bat.recs["metrics"]["eth_protocol"] == 0x86DD)
    for have in (bat.recs["id"]["src_ip"][v6], bat.recs["id"]["dst_ip"][v6], bat.parts["xlat"]["saddr"][addr], bat.parts["xlat"]["daddr"][addr]):
        assert want <= {a.tobytes() for a in have}
    for p in range(256):
        assert tc.partner(p) != p
    assert sorted(tc.partner(p) for p in range(256)) == sorted(tc.xlat_partner(p) for p in range(256)) == list(range(256))
    assert tc.xlat_partner(0) == 0
    # both ip_text calls of a lane differ, in every pattern record
    n = 256 * 3
    assert all(tc.pattern_of(bat.recs["id"]["src_ip"][k].tobytes()) != tc.pattern_of(bat.recs["id"]["dst_ip"][k].tobytes()) for k in range(n))


def test_the_26_tie_patterns(bat):
    """Counted here from the text of the bits, not with textcraft's own run finder."""
    ties = []
    for p in range(256):
        bits = "".join("1" if (p >> k) & 1 else "0" for k in range(8))
        runs = [len(r) for r in re.findall("00+", bits)]
        if runs and runs.count(max(runs)) >= 2:
            ties.append(p)
    assert len(ties) == 26 and ties == tc.tie_patterns()
    src = {tc.pattern_of(a.tobytes()) for a in bat.recs["id"]["src_ip"][bat.family == "addr"][:768]}
    assert set(ties) <= src
    for p in ties:                                            # "the first one": the text has its "::" where the first of the tied runs stands
        bits = "".join("1" if (p >> k) & 1 else "0" for k in range(8))
        first = re.search("0" * max(len(r) for r in re.findall("00+", bits)), bits).start()
        text = R.go_ip(tc.addr_of(p, "one")).decode()
        assert text.index("::") == len(":".join(["1"] * first)) if first else text.startswith("::"), (p, text)
    for cls in tc.WIDTH_CLASSES:
        assert R.go_ip(tc.addr_of(0b10000000, cls)).startswith(b"::") and R.go_ip(tc.addr_of(0, cls)) == b"::"


def test_v4_mapped_octets_and_the_near_misses(bat):
    addr = bat.recs[bat.family == "addr"]
    v4 = addr[addr["metrics"]["eth_protocol"] == 0x0800]
    for side in ("src_ip", "dst_ip"):
        mapped = [a.tobytes() for a in v4["id"][side] if a.tobytes()[:12] == tc.V4MAP]
        for o in range(4):
            assert {a[12 + o] for a in mapped} >= set(tc.OCTETS), (side, o)
    texts = {(R.go_ip(s), R.go_ip(d), e) for s, d, e in tc.near_misses()}
    assert (b"::fffe:a00:9ff", b"::feff:a00:9ff", 0x86DD) in texts                       # bytes 10-11 = ff fe
    assert any(s.endswith(b":ffff:a00:9ff") and s[:1] != b":" for s, _, _ in texts)       # a non-zero byte in front of ff ff
    assert (b"0.0.0.0", b"10.0.9.255", 0x86DD) in texts                                  # ::ffff:0:0 under the IPv6 ethertype
    assert any(e == 0x0800 and b":" in s and b":" in d for s, d, e in texts)             # unmapped under the IPv4 ethertype
    have = {(a["id"]["src_ip"].tobytes(), a["id"]["dst_ip"].tobytes(), int(a["metrics"]["eth_protocol"])) for a in addr}
    assert set(tc.near_misses()) <= have


def test_go_ip_equals_ipaddress_on_every_battery_address(bat):
    addrs = set()
    for a in (bat.recs["id"]["src_ip"], bat.recs["id"]["dst_ip"], bat.parts["xlat"]["saddr"], bat.parts["xlat"]["daddr"]):
        addrs |= {x.tobytes() for x in a}
    assert len(addrs) > 780                                  # the 766 pattern addresses are the same set on all four sides
    for a in addrs:
        ip = ipaddress.IPv6Address(a)
        want = str(ip.ipv4_mapped) if ip.ipv4_mapped is not None else str(ip)
        assert R.go_ip(a) == want.encode(), a.hex()


def _values(lines, key):
    out = set()
    for ln in lines:
        for mm in re.finditer(rb'"%s":(-?\d+)[,}]' % key.encode(), ln):
            out.add(int(mm.group(1)))
    return out


def test_every_listed_edge_of_every_field_is_in_the_lines(nf, dt):
    d = tc.family(*dt, "digits")
    tls = T.table_of(nf.GO_TLS_NAMES)
    lines = lines_of(d, tc.CLOCKS[0], tls)
    assert len(lines) == len(d.recs)
    for key, width in tc.FIELD_WIDTH.items():
        want = {v for v in tc.EDGES[width] if v or key not in tc.GATED}
        assert set(tc.DECIMAL_EDGES[width]) - {0} <= set(tc.EDGES[width])
        assert want <= _values(lines, key), (key, sorted(want - _values(lines, key)))
    dirs = [set() for _ in range(7)]
    for ln in lines:
        for k, v in enumerate(re.search(rb'"IfDirections":\[([\d,]*)\]', ln).group(1).split(b",")):
            dirs[k].add(int(v))
    assert all(s >= set(tc.EDGES[3]) for s in dirs)                                      # the seven IfDirections, each position
    blob = b"\n".join(lines)
    for v in tc.EDGES[10]:
        assert b'"QuicVersion":"QUIC Unknown (%d)"' % v in blob, v
    for v in tc.EDGES[5]:
        if v:
            assert (T.GROUP, v) not in tls and b'"TLSGroup":"CurveID(%d)"' % v in blob, v
    for v in tc.TLS_FALLBACK_IDS:
        assert (T.VERSION, v) not in tls and (b'"TLSVersion":"0x%04X"' % v in blob or b'"TLSVersion":"~ 0x%04X"' % v in blob), v
    assert sum((T.CIPHER_SUITE, v) not in tls and b'"TLSCipherSuite":"0x%04X"' % v in blob for v in tc.TLS_FALLBACK_IDS) >= 4
    for key in (b"SrcMac", b"DstMac"):                                                   # each byte position, both nibbles: 0, 9, a, f
        macs = [re.search(rb'"%s":"([0-9a-f:]{17})"' % key, ln).group(1).split(b":") for ln in lines]
        for pos in range(6):
            assert {m[pos][:1] for m in macs} >= {b"0", b"9", b"a", b"f"} <= {m[pos][1:] for m in macs}, (key, pos)
    # signed values, as the parts hold them -> as Go prints them
    i64 = tc.wrap_i64
    assert {i64(v) for v in tc.RTT} <= _values(lines, "TimeFlowRttNs") and set(tc.RET) <= _values(lines, "IPSecRetCode")
    assert {math.trunc(fractions.Fraction(i64(v), 10**6)) for v in tc.LATENCY} <= _values(lines, "DnsLatencyMs")
    assert {I for I in (tc.I64_MIN, tc.I64_MAX, -1)} <= {i64(v) for v in tc.RTT}
    assert {-2**31, 2**31 - 1, 1, -1, 10**9, -10**9} <= set(tc.RET)
    # each branch of the line is live on some record
    for text in (b'"SrcPort":', b'"Flags":', b'"IcmpType":', b'"Proto":132', b'"Proto":17', b'"Etype":9,', b'"PktDropLatestDropCause":"OVS_DROP_'):
        assert text in blob, text


def test_the_printed_decimals_are_the_integers_of_the_records(nf, dt):
    d = tc.family(*dt, "digits")
    lines = lines_of(d, tc.CLOCKS[0], T.table_of(nf.GO_TLS_NAMES))
    m, a, dns = d.recs["metrics"], d.parts["additional"], d.parts["dns"]
    for k, ln in enumerate(lines):
        for key, v in ((b"Bytes", int(m["bytes"][k])), (b"Packets", int(m["packets"][k])), (b"Sampling", int(m["sampling"][k])), (b"Etype", int(m["eth_protocol"][k])),
                       (b"TimeFlowRttNs", tc.wrap_i64(int(a["flow_rtt"][k]))), (b"IPSecRetCode", int(a["ipsec_encrypted_ret"][k])),
                       (b"DnsLatencyMs", math.trunc(fractions.Fraction(tc.wrap_i64(int(dns["latency"][k])), 10**6)))):
            assert b'"%s":%s,' % (key, str(v).encode()) in ln, (k, key, v)


def test_unix_milli_is_floor_division_on_every_clock_case():
    names = set()
    for clock in tc.CLOCKS:
        now, mono = tc.now_of(clock), clock[2]
        for name, ts in tc.clock_cases(clock):
            names.add(name)
            d = tc.wrap_i64(-tc.wrap_i64(mono - ts))
            assert R.unix_milli(now, mono, ts) == (now + d) // 10**6, (clock, name)
    assert len(names) == 15


def test_the_clock_family_has_both_carries_the_boundaries_and_a_change_of_sign():
    """Computed from the cases, as time.Time.Add computes: Go's % keeps the sign of d."""
    G = 10**9
    up = down = 0
    sums, nsecs, walls, ms = set(), set(), set(), set()
    for clock in tc.CLOCKS:
        now_sec, nsec, mono, _ = clock
        assert 0 <= nsec < G
        for name, ts in tc.clock_cases(clock):
            d = tc.wrap_i64(ts - mono)
            rem = int(math.fmod(d, G)) if abs(d) < 2**53 else d - G * (abs(d) // G) * (1 if d > 0 else -1)
            s = nsec + rem
            sums.add(s)
            up, down = up + (s >= G), down + (s < 0)
            nsecs.add(s % G)
            walls.add(tc.now_of(clock) + d)
            ms.add(R.unix_milli(tc.now_of(clock), mono, ts))
            if name == "delta 2^63":
                assert d == tc.I64_MIN
    assert up >= len(tc.CLOCKS) and down >= len(tc.CLOCKS)
    assert {G - 1, G, 0, -1} <= sums and {999_999, 1_000_000, 0, G - 1} <= nsecs and {-1, 0, 1} <= walls
    assert any(v < 0 for v in ms) and any(v > 0 for v in ms) and {-1, 0} <= ms            # wall -1 ns is millisecond -1, not 0
    assert {c[1] for c in tc.CLOCKS} == {0, 1, 500_000_000, 999_999_999}
    assert any(c[0] > 0 for c in tc.CLOCKS) and any(c[0] == 0 for c in tc.CLOCKS) and any(c[0] < 0 for c in tc.CLOCKS)
    assert {0, -1, tc.I64_MIN, tc.I64_MAX} <= {c[3] for c in tc.CLOCKS}
    for clock in tc.CLOCKS:
        ts = dict(tc.clock_cases(clock))
        assert ts["ts 0"] == 0 and ts["ts 2^64 - 1"] == tc.M64 and ts["delta 0"] == clock[2]


def test_hash_ids_have_every_hex_width(bat):
    assert {len("%x" % v) for v in tc.HASH_IDS} == set(range(1, 17)) and {0, 1, 0xf, 0x10, tc.M64} <= set(tc.HASH_IDS)
    h = bat.family == "hash_id"
    assert bat.ids[h].tolist() == tc.HASH_IDS
    m, i = bat.recs["metrics"][h], bat.recs["id"][h]
    assert np.isin(m["eth_protocol"], (0x0800, 0x86DD)).all() and np.isin(i["transport_protocol"], (6, 17, 132)).all()     # tracked flows


def test_sizes_and_arrangements(dt, bat):
    n = len(bat.recs)
    assert 850 <= n <= 1100 and set(bat.family.tolist()) == set(tc.FAMILIES)
    want = sorted(r.tobytes() for r in bat.recs)
    inter = tc.arrange(bat, "interleaved", *dt)
    assert sorted(r.tobytes() for r in inter.recs) == want and len(inter.recs) == n
    assert (inter.family[1:] != inter.family[:-1]).mean() > 0.25                          # neighbouring lanes of different families
    same = sum(inter.recs[k].tobytes() == bat.recs[k].tobytes() for k in range(n))
    assert same < 8
    grouped = tc.arrange(bat, "grouped", *dt)
    assert len(grouped.recs) % 64 == 0 and len(grouped.recs) <= 4000
    assert all(len(set(grouped.family[w:w + 64].tolist())) == 1 for w in range(0, len(grouped.recs), 64))
    assert {r.tobytes() for r in grouped.recs} == set(want)
    odd = tc.arrange(bat, "odd lane", *dt)
    assert len(odd.recs) == 64 * tc.ODD_WAVES <= 4000
    at = np.flatnonzero(odd.family != "plain")
    assert (at // 64).tolist() == list(range(tc.ODD_WAVES)) and set((at % 64).tolist()) == set(tc.ODD_LANES)
    assert set(odd.family[at].tolist()) == set(tc.FAMILIES)
    base = tc.plain(*dt, 1)
    assert all(odd.recs[k].tobytes() == base.recs[0].tobytes() for k in np.flatnonzero(odd.family == "plain"))
    chosen = {tc.pattern_of(odd.recs["id"]["src_ip"][k].tobytes()) for k in at if odd.family[k] == "addr"}
    assert chosen == set(tc.tie_patterns())
    for b in (inter, grouped, odd):
        assert len(b.present) == len(b.ids) == len(b.family) == len(b.recs) and all(len(v) == len(b.recs) for v in b.parts.values())


def test_the_battery_closes_what_the_seeded_stream_leaves_open(nf, O, bat, capsys):
    """The stream of tests/test_flp_json_gpu.py at its largest size next to the battery, on textcraft.coverage's counts."""
    import test_flp_json_gpu as G
    old, new = tc.coverage(G.stream(nf, O, 50_000, seed=50_001)), tc.coverage(bat.recs)
    with capsys.disabled():
        print("\nvalue shapes reached: seeded stream n = 50 000: %r; battery n = %d: %r" % (old, len(bat.recs), new))
    assert new["patterns"] == 256 and new["ties"] == 26 and new["edges"] == new["edges_of"]
    assert old["patterns"] < 256 and old["ties"] < 26 and old["edges"] < old["edges_of"] // 4
