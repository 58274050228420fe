"""MapTracer flow -> direct-FLP JSON line on the GPU (csrc/nfagg_flp_content.hip) through the C ABI, host and device entry
points: byte parity with the restatement of tests/flp_json_content_ref.py on seeded streams with every part present on
about half the flows, equivalence with nfagg_encode_flp_json when no flow has a part, worst-case lines, missing part arrays,
truncation and the size query, deferred records, the LDS staging limit of the namer table, and the drained maps merged and
encoded without leaving HBM. The records, the namer table and the comparison are those of tests/test_flp_json_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_content_ref as R  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
from test_map_merge import make_maps  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES, NOW, MONO, RECEIVED, AGENT = G.NAMES, G.NOW, G.MONO, G.RECEIVED, G.AGENT
KINDS = ("additional", "dns", "drops", "xlat", "quic")
V4MAP = bytes(10) + b"\xff\xff"
DNS_NAMES = [b"", b"\x03www\x07example\x03com", b"\x01a", b"\x1f" + b"\x01" * 31, b'\x05"\\\t\n\r\x02\x80\xff', b"\xc0\x0c", b"\x03ab",
             b"\x02ab\xc0\x0c", b"\x0fabcdefghijklmno\x0fabcdefghijklmno", b"\x1f" + b"x" * 31, b"\x07ex\x00mple"]


def _choice(rng, values, n, dtype):
    return np.array(values, dtype=dtype)[rng.integers(0, len(values), n)]


def content_parts(nf, n, seed):
    """present + the five part arrays for n flows: each part on about half the flows, independently (and the network-event
    bit on some); every byte random first (time stamps, ethertype, padding), then every field a rule looks at drawn so that
    its gate is closed on some flows and its extremes occur."""
    rng = np.random.default_rng(seed)
    parts = {}
    for k in KINDS:
        a = np.zeros(n, dtype=nf.ROLLUP_KINDS[k])
        a.view(np.uint8).reshape(n, a.dtype.itemsize)[:] = rng.integers(0, 256, (n, a.dtype.itemsize), dtype=np.uint8)
        parts[k] = a
    d = parts["dns"]
    d["id"] = _choice(rng, [0, 1, 7, 65535], n, np.uint16)
    d["errno_"] = _choice(rng, [0, 0, 1, 110, 255], n, np.uint8)
    d["latency"] = _choice(rng, [0, 1, 999_999, 10_000_000, 2**63, 2**64 - 1, 2**64 - 1_500_000, 123_456_789_012], n, np.uint64)
    names = np.zeros((len(DNS_NAMES) + 1, 32), dtype=np.uint8)
    for k, nm in enumerate(DNS_NAMES):
        names[k, :len(nm)] = np.frombuffer(nm, dtype=np.uint8)
    pick = rng.integers(0, len(DNS_NAMES) + 1, n)
    keep_random = pick == len(DNS_NAMES)                                   # the rest keep 32 random bytes: no NUL needed
    d["name"][~keep_random] = names[pick[~keep_random]]
    p = parts["drops"]
    p["latest_drop_cause"] = _choice(rng, [0, 0, 1, 2, 5, 13, 48, 80, 81, 3 << 16, (3 << 16) + 1, (3 << 16) + 11, (3 << 16) + 12, 1 << 24,
                                           (1 << 24) + 3, (1 << 24) + 9, (1 << 24) + 10, 2**32 - 1], n, np.uint32)
    some = rng.integers(0, 4, n) == 0
    p["latest_drop_cause"][some] = rng.integers(2, 81, int(some.sum()))
    p["latest_state"] = rng.integers(0, 14, n)
    x = parts["xlat"]
    for f in ("saddr", "daddr"):
        kind = rng.integers(0, 6, n)
        x[f][kind == 0] = 0
        x[f][kind == 1] = np.frombuffer(V4MAP + bytes(4), dtype=np.uint8)
        x[f][kind == 2, :12] = np.frombuffer(V4MAP, dtype=np.uint8)
        x[f][kind == 3] = x[f][kind == 3] * (rng.integers(0, 3, (int((kind == 3).sum()), 16)) == 0)   # sparse v6 groups
    x["sport"][rng.integers(0, 3, n) == 0] = 0
    x["dport"][rng.integers(0, 3, n) == 0] = 0
    a = parts["additional"]
    a["ipsec_encrypted_ret"] = _choice(rng, [0, 0, 0, -1, 5, -2**31, 2**31 - 1], n, np.int32)
    a["ipsec_encrypted"] = _choice(rng, [0, 1, 2], n, np.uint8)
    a["flow_rtt"] = _choice(rng, [0, 1, 10_000_000, 2**63, 2**64 - 1, 987_654_321_987], n, np.uint64)
    parts["quic"]["version"] = _choice(rng, [0, 1, 2, 0xFFFFFFFF, 0x6B3343CF], n, np.uint32)
    present = np.zeros(n, dtype=np.uint8)
    for k in KINDS + ("network_events",):
        present |= (rng.integers(0, 2, n) * R.FEAT[k]).astype(np.uint8)
    return present, parts


def device_encode(nf, tab, recs, present, parts, names, agent=AGENT, received=RECEIVED, unknown=b"unknown", now=NOW, mono=MONO):
    """Size query, then the write, through the device entry point. present=None: features == NULL."""
    import torch
    n = len(recs)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_recs = dev(recs) if n else None
    d_present = dev(present) if present is not None and n else None
    d_parts = {k: dev(v) for k, v in (parts or {}).items()} if n else {}
    ptrs = {k: v.data_ptr() for k, v in d_parts.items()}
    args = (d_recs.data_ptr() if n else 0, n, d_present.data_ptr() if d_present is not None else 0, ptrs, now, mono, names, agent, received)
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_def = torch.full((max(n, 1),), 0xCD, dtype=torch.uint8, device="cuda")
    rc, need, n_def = tab.encode_flp_json_content_device(*args, 0, 0, d_off.data_ptr(), unknown=unknown)
    assert rc == (nf.TRUNCATED if n else nf.OK)
    d_out = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    rc, wrote, n_def2 = tab.encode_flp_json_content_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), d_def.data_ptr(), unknown=unknown)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert rc == nf.OK and wrote == need and n_def2 == n_def and (out[need:] == 0xAB).all()
    deferred = d_def.cpu().numpy()[:n]
    assert int(deferred.sum()) == n_def
    return out[:need], d_off.cpu().numpy(), deferred


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1025, 20_000])
def test_stream_parity_with_restatement(nf, O, tab, n):
    recs = G.stream(nf, O, n, seed=n + 3)
    present, parts = content_parts(nf, n, seed=n + 5)
    want = R.encode(recs, present, parts, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
    if n >= 1023:
        for k in KINDS:
            have = (present & R.FEAT[k]) != 0
            assert 0.4 * n < have.sum() < 0.6 * n
        for key in (b'"DnsErrno"', b'"DnsName"', b'"DnsLatencyMs":-', b'"IPSecStatus":"error"', b'"IPSecStatus":"success"', b'"PktDropBytes"',
                    b'"NetworkEvent_', b'"SKB_DROP_UNKNOWN_CAUSE"', b'"QUIC Unknown (', b'"TimeFlowRttNs":-', b'"XlatSrcPort"', b'"ZoneId"'):
            assert key in want[0], key
        lens = np.diff(want[1].astype(np.int64))
        assert lens.max() > 3000 and lens.min() < 400
    G.check(tab.encode_flp_json_content(recs, present, parts, NOW, MONO, G.table(nf, NAMES), AGENT, RECEIVED), want)
    G.check(device_encode(nf, tab, recs, present, parts, G.table(nf, NAMES)), want)


def test_no_feature_equals_the_plain_encoder(nf, O, tab):
    """features == NULL and an all-zero present array: the bytes of nfagg_encode_flp_json on the same records."""
    recs = G.stream(nf, O, 3000, seed=21, keep_tls=True)
    _, parts = content_parts(nf, 3000, seed=22)
    names = G.table(nf, NAMES)
    plain = tab.encode_flp_json(recs, NOW, MONO, names, AGENT, RECEIVED)
    assert plain[2].sum() > 0 and len(plain[0]) > 3000 * 300
    G.check(plain, R.encode(recs, None, None, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED))
    zeros = np.zeros(3000, dtype=np.uint8)
    only_events = np.full(3000, R.FEAT["network_events"], dtype=np.uint8)
    for present, p in ((None, None), (zeros, parts), (zeros, {}), (only_events, parts)):
        for got in (tab.encode_flp_json_content(recs, present, p, NOW, MONO, names, AGENT, RECEIVED), device_encode(nf, tab, recs, present, p, names)):
            assert got[0].tobytes() == plain[0].tobytes()
            assert np.asarray(got[1]).astype(np.uint64).tolist() == plain[1].tolist() and got[2].tolist() == plain[2].tolist()


def test_worst_case_lines(nf, O, tab):
    """130 flows, each with seven 16-byte names and 63-byte UDNs and a 31-byte DNS name that all escape six-fold, every part
    present with its longest values: longer than any line of the plain encoder, several windows per wave."""
    n = 130
    recs = G.stream(nf, O, n, seed=31)
    m = recs["metrics"]
    m["if_index_first_seen"], m["nb_observed_intf"], m["observed_intf"] = 7, 6, 7
    m["eth_protocol"], recs["id"]["transport_protocol"] = 0x86DD, 6
    recs["id"]["src_port"] = recs["id"]["dst_port"] = 65535
    recs["id"]["src_ip"] = recs["id"]["dst_ip"] = np.frombuffer(bytes.fromhex("1111222233334444555566667777888f"), dtype=np.uint8)
    m["bytes"], m["packets"], m["sampling"], m["dscp"], m["flags"], m["tls_types"] = 2**64 - 1, 2**32 - 1, 2**32 - 1, 255, 65535, 63
    m["start_mono_time_ts"] = m["end_mono_time_ts"] = 0
    present, parts = content_parts(nf, n, seed=32)
    present[:] = 0x3F
    d, p, x, a, q = (parts[k] for k in ("dns", "drops", "xlat", "additional", "quic"))
    d["id"], d["flags"], d["errno_"], d["latency"] = 65535, 0xFFFB, 255, 2**63
    d["name"] = np.frombuffer(b"\x1f" + b"\x01" * 31, dtype=np.uint8)
    p["bytes"], p["packets"], p["latest_flags"], p["latest_state"], p["latest_drop_cause"] = 65535, 65535, 65535, 0, 13
    x["saddr"] = x["daddr"] = recs["id"]["src_ip"][0]
    x["sport"], x["dport"], x["zone_id"] = 65535, 65535, 65535
    a["ipsec_encrypted_ret"], a["flow_rtt"] = -2**31, 2**63
    q["version"], q["seen_long_hdr"], q["seen_short_hdr"] = 0xFFFFFFFF, 255, 255
    agent = bytes.fromhex("1111222233334444555566667777888f")
    want = R.encode(recs, present, parts, -10**17, MONO, G.rows(NAMES), agent, -2**62)
    lens = np.diff(want[1].astype(np.int64))
    assert lens.min() > 4088                                      # longer than any line the plain encoder can write
    G.check(tab.encode_flp_json_content(recs, present, parts, -10**17, MONO, G.table(nf, NAMES), agent, -2**62), want)
    G.check(device_encode(nf, tab, recs, present, parts, G.table(nf, NAMES), agent, -2**62, now=-10**17), want)


@pytest.mark.parametrize("missing", KINDS)
def test_null_part_array_with_its_bit_set_is_an_absent_part(nf, O, tab, missing):
    recs = G.stream(nf, O, 700, seed=41)
    present, parts = content_parts(nf, 700, seed=42)
    present |= R.FEAT[missing]
    given = {k: v for k, v in parts.items() if k != missing}
    want = R.encode(recs, present, given, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
    assert want[0] != R.encode(recs, present, parts, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)[0]
    G.check(tab.encode_flp_json_content(recs, present, given, NOW, MONO, G.table(nf, NAMES), AGENT, RECEIVED), want)
    G.check(device_encode(nf, tab, recs, present, given, G.table(nf, NAMES)), want)


def test_truncated_then_written(nf, O, tab):
    import torch
    n = 300
    recs = G.stream(nf, O, n, seed=51, keep_tls=True)
    present, parts = content_parts(nf, n, seed=52)
    names = G.table(nf, NAMES)
    want, want_off, want_def = R.encode(recs, present, parts, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
    # host entry point: one byte short
    o, keep = nf.flp_options(NOW, MONO, names, AGENT, RECEIVED)
    feat, keep_f = tab._pb_features(n, present, parts)
    need, n_def = C.c_size_t(0), C.c_size_t(0)
    small = np.full(len(want) - 1, 0xAB, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    flags = np.full(n, 0xCD, dtype=np.uint8)
    call = lambda buf, cap: nf._lib.lib.nfagg_encode_flp_json_content(  # noqa: E731
        tab._h, recs.ctypes.data_as(C.c_void_p), n, C.byref(feat), C.byref(o), buf.ctypes.data_as(C.c_void_p) if buf is not None else None, cap,
        off.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p), C.byref(n_def), C.byref(need))
    assert call(small, len(small)) == nf.TRUNCATED and need.value == len(want) and n_def.value == int(want_def.sum()) > 0
    assert (small == 0xAB).all() and not off.any() and (flags == 0xCD).all()
    full = np.full(len(want), 0xAB, dtype=np.uint8)
    assert call(full, len(full)) == nf.OK and need.value == len(want)
    G.check((full, off, flags), (want, want_off, want_def))
    # device entry point: one byte short, the size query, then written
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_recs, d_present, d_parts = dev(recs), dev(present), {k: dev(v) for k, v in parts.items()}
    args = (d_recs.data_ptr(), n, d_present.data_ptr(), {k: v.data_ptr() for k, v in d_parts.items()}, NOW, MONO, names, AGENT, RECEIVED)
    d_out = torch.full((len(want) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_def = torch.full((n,), 0xCD, dtype=torch.uint8, device="cuda")
    rc, got, nd = tab.encode_flp_json_content_device(*args, d_out.data_ptr(), len(want) - 1, d_off.data_ptr(), d_def.data_ptr())
    torch.cuda.synchronize()
    assert rc == nf.TRUNCATED and got == len(want) and nd == int(want_def.sum())
    assert (d_out.cpu().numpy() == 0xAB).all() and not d_off.cpu().numpy().any() and (d_def.cpu().numpy() == 0xCD).all()
    rc, got, nd = tab.encode_flp_json_content_device(*args, 0, 1 << 30, d_off.data_ptr())
    assert rc == nf.TRUNCATED and got == len(want) and not d_off.cpu().numpy().any()          # d_out == NULL: the size
    rc, got, nd = tab.encode_flp_json_content_device(*args, d_out.data_ptr(), len(want), d_off.data_ptr(), d_def.data_ptr())
    torch.cuda.synchronize()
    assert rc == nf.OK and got == len(want) and nd == int(want_def.sum())
    out = d_out.cpu().numpy()
    assert (out[len(want):] == 0xAB).all()
    G.check((out[: len(want)], d_off.cpu().numpy(), d_def.cpu().numpy()), (want, want_off, want_def))


def test_deferred_records_among_content_flows(nf, O, tab):
    recs = G.stream(nf, O, 5000, seed=61, keep_tls=True)
    present, parts = content_parts(nf, 5000, seed=62)
    m = recs["metrics"]
    mask = ((m["ssl_version"] != 0) | (m["tls_cipher_suite"] != 0) | (m["tls_key_share"] != 0)).astype(np.uint8)
    assert 0 < mask.sum() < len(recs) and (present[mask == 1] != 0).any()
    want = R.encode(recs, present, parts, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
    assert want[2].tolist() == mask.tolist()
    for got in (tab.encode_flp_json_content(recs, present, parts, NOW, MONO, G.table(nf, NAMES), AGENT, RECEIVED),
                device_encode(nf, tab, recs, present, parts, G.table(nf, NAMES))):
        lens = np.diff(np.asarray(got[1]).astype(np.int64))
        assert got[2].tolist() == mask.tolist() and (lens[mask == 1] == 0).all() and (lens[mask == 0] > 0).all()
        G.check(got, want)


def test_namer_table_larger_than_lds(nf, O, tab):
    names = [(1000 + k, None, "if%d" % k, "udn%d" % k if k % 3 else "") for k in range(150)] + NAMES
    recs = G.stream(nf, O, 3000, seed=71)
    recs["metrics"]["if_index_first_seen"][::2] = 1000 + (np.arange(1500) % 150)
    recs["metrics"]["observed_intf"][::4, 1] = 1000 + (np.arange(750) % 150)
    present, parts = content_parts(nf, 3000, seed=72)
    G.check(tab.encode_flp_json_content(recs, present, parts, NOW, MONO, G.table(nf, names), AGENT, RECEIVED, b"?"),
            R.encode(recs, present, parts, NOW, MONO, G.rows(names), AGENT, RECEIVED, b"?"))


def test_drained_maps_merged_and_encoded_on_the_device(nf, O, tab):
    """nfagg_map_merge_device (main map and all six feature maps, 4 CPUs) -> nfagg_encode_flp_json_content_device on its d_out,
    against the restatement over what the host nfagg_map_merge returns for the same maps."""
    import torch
    n_cpu = 4
    mi, mv, feats = make_maps(O, 81, 6000, 3500, 2500, n_cpu)
    raw = mv.view(np.uint8).reshape(len(mv), 104)
    keep = np.arange(len(mv)) % 5 == 0
    raw[~keep, 92:98] = 0                                         # ssl_version, tls_cipher_suite, tls_key_share: most flows not deferred
    h_recs, h_present, h_parts, n_dup = tab.map_merge(mi, mv, feats, n_cpu)
    assert n_dup == 0 and len(h_recs) > 3500 and all((h_present & R.FEAT[k]).any() for k in KINDS + ("network_events",))
    want = R.encode(h_recs, h_present, h_parts, NOW, MONO, G.rows(NAMES), AGENT, RECEIVED)
    assert 0 < want[2].sum() < len(h_recs) / 2
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_mi, d_mv = dev(mi), dev(mv)
    d_f = {k: (dev(a), dev(b), len(a)) for k, (a, b) in feats.items()}
    total = len(mi) + sum(len(a) for a, _ in feats.values())
    sizes = {"records": 144, "present": 1, "additional": 32, "dns": 64, "drops": 32, "network_events": 72, "xlat": 56, "quic": 24}
    d_m = {k: torch.zeros(total * s + 16, dtype=torch.uint8, device="cuda") for k, s in sizes.items()}
    rc, n, n_dup = tab.map_merge_device((d_mi.data_ptr(), d_mv.data_ptr(), len(mi)), {k: (i.data_ptr(), v.data_ptr(), c) for k, (i, v, c) in d_f.items()},
                                        n_cpu, {k: t.data_ptr() for k, t in d_m.items()}, total)
    assert rc == nf.OK and n == len(h_recs)
    args = (d_m["records"].data_ptr(), n, d_m["present"].data_ptr(), {k: d_m[k].data_ptr() for k in KINDS + ("network_events",)}, NOW, MONO,
            G.table(nf, NAMES), AGENT, RECEIVED)
    d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_def = torch.empty(n, dtype=torch.uint8, device="cuda")
    rc, need, nd = tab.encode_flp_json_content_device(*args, 0, 0, d_off.data_ptr())
    assert rc == nf.TRUNCATED and need == len(want[0])
    d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    rc, wrote, nd = tab.encode_flp_json_content_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), d_def.data_ptr())
    assert rc == nf.OK and wrote == need and nd == int(want[2].sum())
    G.check((d_out[:need].cpu().numpy(), d_off.cpu().numpy(), d_def.cpu().numpy()), want)
