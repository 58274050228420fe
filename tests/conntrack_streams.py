"""What the conversation-tracking tests share beside the restatement: a seeded record stream that needs no GPU test module and no
oracle, and the table's home slot restated for the crafted collisions."""
import numpy as np

M64 = (1 << 64) - 1


def fmix64(x: int) -> int:
    """MurmurHash3's 64-bit finalizer: nfagg_conn_fold probes from its low bits (include/nfagg.h)."""
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    return x ^ (x >> 33)


def home_slot(total: int, slots: int = 1024) -> int:
    return fmix64(total) & (slots - 1)


def seeded_records(nf, n: int, seed: int):
    """n records: IPv4 (v4-mapped), IPv6 with sparse groups, IPv4 ethertype over unmapped addresses, a non-IP ethertype; protocols
    1 / 6 / 17 / 58 / 132 / 47 / 0; ports on both sides of 128 and 256; random flags, bytes up to 2^40, zero bytes and packets."""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=nf.FLOW_RECORD)
    k, m = r["id"], r["metrics"]
    fam = rng.choice(4, n, p=[0.45, 0.35, 0.1, 0.1])                        # v4, v6, 0x0800 with unmapped addresses, ARP
    for side in ("src_ip", "dst_ip"):
        a = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        sparse = (rng.integers(0, 3, (n, 16)) > 0) & (rng.integers(0, 2, (n, 1)) > 0)
        a = np.where(sparse, a, 0).astype(np.uint8)
        v4 = fam == 0
        a[v4, :10], a[v4, 10:12] = 0, 0xFF
        k[side] = a
    m["eth_protocol"] = np.choose(fam, [0x0800, 0x86DD, 0x0800, 0x0806])
    k["transport_protocol"] = rng.choice(np.array([1, 6, 6, 17, 58, 132, 47, 0], dtype=np.uint8), n)
    for side in ("src_port", "dst_port"):
        k[side] = rng.choice(np.array([0, 1, 53, 127, 128, 255, 256, 443, 8080, 65535], dtype=np.uint16), n)
    m["flags"] = rng.choice(np.array([0, 0x10, 0x11, 0x112, 0x01, 0x02, 0xFFFF], dtype=np.uint16), n)
    m["bytes"] = rng.integers(0, 1 << 40, n, dtype=np.uint64) * (rng.integers(0, 5, n) > 0)
    m["packets"] = rng.integers(0, 1 << 20, n, dtype=np.uint32) * (rng.integers(0, 5, n) > 0)
    m["start_mono_time_ts"] = rng.integers(0, 1 << 42, n, dtype=np.uint64)
    m["end_mono_time_ts"] = rng.integers(0, 1 << 42, n, dtype=np.uint64)
    return r
