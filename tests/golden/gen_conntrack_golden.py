"""Writes conntrack_vectors.json and conntrack_collisions.json beside itself (data only; run once, by hand: `python gen_conntrack_golden.py`).

conntrack_vectors.json
  tuples   endpoint tuples with the gob message of every field (hex) and the three FNV-64a hashes. The messages of the first
           rows are the worked examples of encoding/gob's format ("10.0.0.1" -> 0b 0c 00 08 31 30 2e 30 2e 30 2e 31, port 80 ->
           03 06 00 50, port 443 -> 05 06 00 fe 01 bb, Proto 6 -> 03 06 00 06); the hashes are computed HERE, by the few lines
           below, not by tests/conntrack_ref.py.
  traces   state traces worked by hand: per call a clock, flows, and the records Extract must return, each as one line
           "<type> <SrcAddr>:<SrcPort>><DstAddr>:<DstPort> n=<numFlowLogs> ab=<Bytes_AB> ba=<Bytes_BA> first=<_IsFirst>"
           (a flowLog record: "flowLog <SrcAddr>:<SrcPort>><DstAddr>:<DstPort>"). The expectations are literals of this file.

conntrack_collisions.json: endpoint tuples found by a search over 2^22 tuples (src 10.1.2.3, dst 10.9.8.7, TCP, 2 048 x 2 048 ports
from 1024 on, so that every gob message has one length) with a vectorised FNV-64a:
  same_home   twenty connections whose home slot in the smallest table (1 024 slots: the low ten bits of fmix64(hashTotal)) is
              one slot;
  same_word0  pairs of connections whose totals share the upper 32 bits, the table's first key word, AND the home slot in the
              smallest table, so that the second to arrive finds the first word of its home slot equal to its own and must tell
              the connections apart by the second word. A birthday on 32 bits: 2^22 tuples hold about 2^44 / 2^33 = 2 048 pairs
              with an equal upper word, and one in 1 024 of those shares the home slot: about two."""
import json
import os

import numpy as np

M64 = (1 << 64) - 1
OFFSET, PRIME = 0xcbf29ce484222325, 0x100000001b3


def fnv(data, h=OFFSET):
    for b in data:
        h = ((h ^ b) * PRIME) & M64
    return h


def uint_msg(v):
    if v < 128:
        return bytes([3, 6, 0, v])
    if v < 256:
        return bytes([4, 6, 0, 0xff, v])
    return bytes([5, 6, 0, 0xfe, v >> 8, v & 255])


def str_msg(s):
    return bytes([3 + len(s), 0x0c, 0, len(s)]) + s.encode()


def hashes(src, sport, dst, dport, proto):
    a, b, c = fnv(str_msg(src) + uint_msg(sport)), fnv(str_msg(dst) + uint_msg(dport)), fnv(uint_msg(proto))
    lo, hi = min(a, b), max(a, b)
    return a, b, fnv(c.to_bytes(8, "big") + lo.to_bytes(8, "big") + hi.to_bytes(8, "big"))


# (src as the record holds it: text of 4 or 16 bytes, src text as net.IP.String() prints it, ...)
TUPLES = [
    ("10.0.0.1", "10.0.0.1", 80, "10.0.0.2", "10.0.0.2", 443, 6),
    ("10.0.0.2", "10.0.0.2", 443, "10.0.0.1", "10.0.0.1", 80, 6),                                   # the other direction
    ("::ffff:192.168.1.10", "192.168.1.10", 127, "::ffff:192.168.1.11", "192.168.1.11", 128, 17),   # v4-mapped; ports around 128
    ("192.168.1.10", "192.168.1.10", 255, "192.168.1.11", "192.168.1.11", 256, 17),                 # ... and around 256
    ("2001:db8:0:0:0:0:0:1", "2001:db8::1", 65535, "2001:db8:0:0:1:0:0:2", "2001:db8::1:0:0:2", 0, 132),   # compressed runs; SCTP
    ("fe80:0:0:0:0:0:0:0", "fe80::", 5353, "ff02:0:0:0:0:0:0:fb", "ff02::fb", 5353, 17),
    ("0:0:0:0:0:0:0:1", "::1", 8080, "0:0:0:0:0:0:0:1", "::1", 8080, 6),                            # src == dst: hashA == hashB
    ("10.255.255.254", "10.255.255.254", 1, "10.0.0.0", "10.0.0.0", 65535, 6),
    ("1:2:3:4:5:6:7:8", "1:2:3:4:5:6:7:8", 1024, "1:0:0:4:0:0:0:8", "1:0:0:4::8", 2048, 6),         # the first LONGEST run
    ("172.16.0.9", "172.16.0.9", 53, "172.16.0.10", "172.16.0.10", 40000, 17),
    ("172.16.0.9", "172.16.0.9", 53, "172.16.0.10", "172.16.0.10", 40000, 6),                        # the same endpoints, another protocol
    ("abcd:ef01:2345:6789:abcd:ef01:2345:6789", "abcd:ef01:2345:6789:abcd:ef01:2345:6789", 443, "a:b:c:d:e:f:0:1", "a:b:c:d:e:f:0:1", 443, 132),
]

A, B, C, D, E, F = ("10.0.0.1", 1000), ("10.0.0.2", 80), ("10.0.0.3", 53), ("10.0.0.4", 5353), ("10.0.0.5", 1), ("10.0.0.6", 2)
S = 10**9


def fl(src, dst, proto=6, nbytes=0, flags=0, packets=1):
    return dict(src=src[0], sport=src[1], dst=dst[0], dport=dst[1], proto=proto, bytes=nbytes, packets=packets, flags=flags)


def line(kind, src, dst, n, ab, ba, first):
    return "%s %s:%d>%s:%d n=%d ab=%d ba=%d first=%s" % (kind, src[0], src[1], dst[0], dst[1], n, ab, ba, first)


def flog(src, dst):
    return "flowLog %s:%d>%s:%d" % (src[0], src[1], dst[0], dst[1])


# scheduling of every trace: UDP {end 5s, terminating 2s, heartbeat 3s}, default {end 10s, terminating 4s, heartbeat 6s}
TRACES = [
    dict(name="new, update, FIN, end after terminatingTimeout", calls=[
        dict(now=0, flows=[fl(A, B, nbytes=100), fl(B, A, nbytes=50)], want=[line("newConnection", A, B, 1, 100, 0, True)]),
        dict(now=1 * S, flows=[fl(A, B, nbytes=10, flags=0x11)], want=[]),
        dict(now=5 * S, flows=[], want=[]),                                     # now.After(expiry) is strict
        dict(now=5 * S + 1, flows=[], want=[line("endConnection", A, B, 3, 110, 50, False)])]),
    dict(name="timeout end", calls=[
        dict(now=0, flows=[fl(A, B, nbytes=100)], want=[line("newConnection", A, B, 1, 100, 0, True)]),
        dict(now=10 * S + 1, flows=[], want=[line("endConnection", A, B, 1, 100, 0, False)])]),
    dict(name="heartbeats", calls=[
        dict(now=0, flows=[fl(A, B, nbytes=100)], want=[line("newConnection", A, B, 1, 100, 0, True)]),
        dict(now=7 * S, flows=[fl(B, A, nbytes=5)], want=[line("heartbeat", A, B, 2, 100, 5, False)]),
        dict(now=13 * S, flows=[], want=[]),
        dict(now=14 * S, flows=[], want=[line("heartbeat", A, B, 2, 100, 5, False)])]),
    dict(name="two scheduling groups by Proto: groups in order, not connections", calls=[
        dict(now=0, flows=[fl(A, B, nbytes=100), fl(C, D, proto=17, nbytes=30)],
             want=[line("newConnection", A, B, 1, 100, 0, True), line("newConnection", C, D, 1, 30, 0, True)]),
        dict(now=11 * S, flows=[], want=[line("endConnection", C, D, 1, 30, 0, False), line("endConnection", A, B, 1, 100, 0, False)])]),
    dict(name="the limit reached mid-call; the flow log of a flow turned away is still written", max_conns=2, flow_logs=True, calls=[
        dict(now=0, flows=[fl(A, B, nbytes=1), fl(C, D, proto=17, nbytes=2), fl(E, F, nbytes=3), fl(B, A, nbytes=4)],
             want=[line("newConnection", A, B, 1, 1, 0, True), flog(A, B), line("newConnection", C, D, 1, 2, 0, True), flog(C, D), flog(E, F), flog(B, A)]),
        dict(now=11 * S, flows=[], want=[line("endConnection", C, D, 1, 2, 0, False), line("endConnection", A, B, 2, 1, 4, False)])]),
    dict(name="swapAB: SYN_ACK in the first flow", calls=[
        dict(now=0, flows=[fl(B, A, nbytes=70, flags=0x112), fl(A, B, nbytes=20, flags=0x10)], want=[line("newConnection", A, B, 1, 0, 70, True)]),
        dict(now=11 * S, flows=[], want=[line("endConnection", A, B, 2, 20, 70, False)])]),
    dict(name="FIN on the very first flow; a terminated connection that reappears", calls=[
        dict(now=0, flows=[fl(A, B, nbytes=10, flags=0x01)], want=[line("newConnection", A, B, 1, 10, 0, True)]),
        dict(now=1 * S, flows=[fl(A, B, nbytes=5)], want=[]),                     # aggregated, but neither expiry moves
        dict(now=4 * S + 1, flows=[], want=[line("endConnection", A, B, 2, 15, 0, False)]),
        dict(now=5 * S, flows=[fl(A, B, nbytes=7)], want=[line("newConnection", A, B, 1, 7, 0, True)])]),
    dict(name="a UDP record with FIN and SYN_ACK bits neither terminates nor swaps", calls=[
        dict(now=0, flows=[fl(C, D, proto=17, nbytes=30, flags=0x101)], want=[line("newConnection", C, D, 1, 30, 0, True)]),
        dict(now=2 * S + 1, flows=[], want=[]),
        dict(now=5 * S + 1, flows=[], want=[line("endConnection", C, D, 1, 30, 0, False)])]),
    dict(name="a heartbeat is the first report when newConnection is off", no_new=True, calls=[
        dict(now=0, flows=[fl(A, B, nbytes=9)], want=[]),
        dict(now=6 * S + 1, flows=[], want=[line("heartbeat", A, B, 1, 9, 0, True)])]),
]


def fmix64(x):
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xff51afd7ed558ccd)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xc4ceb9fe1a85ec53)
    return x ^ (x >> np.uint64(33))


def vfnv(h, byte):
    return (h ^ byte.astype(np.uint64)) * np.uint64(PRIME)


SIDE = 2048


def search():
    """2^22 tuples (10.1.2.3, 1024 + i) -> (10.9.8.7, 1024 + j), TCP: every port message is 05 06 00 fe hi lo."""
    ports = np.arange(1024, 1024 + SIDE, dtype=np.uint64)

    def side(addr):
        h = np.full(SIDE, fnv(str_msg(addr) + bytes([5, 6, 0, 0xfe])), dtype=np.uint64)
        return vfnv(vfnv(h, ports >> np.uint64(8)), ports & np.uint64(255))
    with np.errstate(over="ignore"):
        a, b = np.meshgrid(side("10.1.2.3"), side("10.9.8.7"), indexing="ij")
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        t = np.full(a.shape, fnv(fnv(uint_msg(6)).to_bytes(8, "big")), dtype=np.uint64)
        for w in (lo, hi):
            for k in range(7, -1, -1):
                t = vfnv(t, (w >> np.uint64(8 * k)) & np.uint64(255))
        home = (fmix64(t) & np.uint64(1023)).ravel()
    t = t.ravel()
    best = np.bincount(home.astype(np.int64), minlength=1024).argmax()
    same_home = np.nonzero(home == best)[0][:20]
    top = t >> np.uint64(32)
    order = np.argsort(top, kind="stable")
    eq = np.nonzero((top[order][1:] == top[order][:-1]) & (home[order][1:] == home[order][:-1]))[0]
    pairs = [(int(order[k]), int(order[k + 1])) for k in eq[:4]]

    def tup(ix):
        return dict(src="10.1.2.3", sport=1024 + ix // SIDE, dst="10.9.8.7", dport=1024 + ix % SIDE, proto=6, total="%x" % int(t[ix]), home=int(home[ix]))
    assert len(same_home) == 20 and pairs
    for ix in list(same_home) + [p for pr in pairs for p in pr]:                     # the vectorised FNV against the plain one
        d = tup(int(ix))
        assert hashes(d["src"], d["sport"], d["dst"], d["dport"], 6)[2] == int(t[ix])
    return dict(searched=int(t.size), home_slot=int(best), same_home=[tup(int(i)) for i in same_home], same_word0=[[tup(a), tup(b)] for a, b in pairs])


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    tuples = []
    for raw_s, src, sport, raw_d, dst, dport, proto in TUPLES:
        a, b, t = hashes(src, sport, dst, dport, proto)
        tuples.append(dict(src=raw_s, src_text=src, sport=sport, dst=raw_d, dst_text=dst, dport=dport, proto=proto,
                           gob=[str_msg(src).hex(), uint_msg(sport).hex(), str_msg(dst).hex(), uint_msg(dport).hex(), uint_msg(proto).hex()],
                           hash_a="%x" % a, hash_b="%x" % b, hash_total="%x" % t))
    json.dump(dict(tuples=tuples, traces=TRACES), open(os.path.join(here, "conntrack_vectors.json"), "w"), indent=1)
    json.dump(search(), open(os.path.join(here, "conntrack_collisions.json"), "w"), indent=1)
