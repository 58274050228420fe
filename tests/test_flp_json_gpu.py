"""Record -> direct-FLP JSON lines on the GPU (csrc/nfagg_flp.hip) through the C ABI: byte parity with the restatement of
tests/flp_json_ref.py on seeded streams reshaped to reach every branch, deferred records, the LDS staging limit of the
namer table, truncation, the size query, chained calls, the device-resident path, 1 M flows, the C driver, and configs[0]
end to end against DirectFLPStdout."""
import ctypes as C
import io
import ipaddress
import os
import queue
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# the namer-table cases of test_ipfix_gpu.NAMES (NOT sorted by index, several rows per index, MAC-specific rows, an empty
# name), plus names and UDNs that need each escape, and worst-case rows: 16 and 63 bytes that all escape six-fold
NAMES = [(8, None, "x" * 16, "u" * 63), (3, bytes.fromhex("020000000001"), "veth3a", "udn-blue"), (1, None, "lo", ""),
         (3, None, "veth3", ""), (2, None, "eth0", "default"), (3, None, "veth3-second-any", "never"),
         (3, bytes.fromhex("aabbccddeeff"), "veth3b", "udn-late"), (4, None, "ovn-k8s-mp0", "t"), (6, None, "", "nameless"),
         (2, bytes.fromhex("020000000002"), "eth0-mac", ""),
         (5, None, b'q"b\\\t\n\r\x01\x7f\xc3\xa9\xff', b"udn \"q\" \\ \x1f\x00 \xe2\x82\xac"), (7, None, b"\x01" * 16, b"\x02" * 63)]
NOW, MONO = 1_700_000_000_123_456_789, 2_500_000
RECEIVED = 1_700_000_003
AGENT = bytes(10) + b"\xff\xff" + bytes([10, 1, 2, 3])


def _b(x):
    return x if isinstance(x, bytes) else x.encode()


def rows(names):
    return [(i, m, _b(n), _b(u)) for (i, m, n, u) in names]


def table(nf, names):
    t = np.zeros(len(names), dtype=nf.INTF_NAME)
    for k, (ifx, mac, name, udn) in enumerate(rows(names)):
        t[k]["if_index"] = ifx
        if mac is not None:
            t[k]["mac"], t[k]["has_mac"] = np.frombuffer(bytes(mac), dtype=np.uint8), 1
        t[k]["name_len"], t[k]["udn_len"] = len(name), len(udn)
        raw = t[k:k + 1].view(np.uint8).reshape(-1)                 # "S" fields drop trailing NULs: write the bytes themselves
        raw[12:12 + len(name)] = np.frombuffer(name, dtype=np.uint8)
        raw[29:29 + len(udn)] = np.frombuffer(udn, dtype=np.uint8)
    return t


def stream(nf, O, n, seed, keep_tls=False):
    """Scrambled records (variant 1: interfaces 1..8, both directions, observed lists of 0..6 entries, zero and non-zero
    times, TLS fields) reshaped: v4, v6, eth 0x0800 with unmapped addresses, a non-IP ethertype, protocols
    1/6/17/58/132/47, zero and non-zero bytes / packets / sampling / dscp, wrapped and zero times, Bytes = 2^64 - 1, sparse
    IPv6 groups, worst-case-length lines (interface 7, six observed 7s) in the same wave as short ones."""
    if n == 0:
        return np.zeros(0, dtype=nf.FLOW_RECORD)
    recs = O.gen_stream(n, seed=seed, n_keys=997, variant=1).view(nf.FLOW_RECORD)
    m, ids = recs["metrics"], recs["id"]
    rng = np.random.default_rng(seed)
    clear = np.arange(n) % 3 != 0 if keep_tls else np.ones(n, dtype=bool)             # keep_tls: every third record keeps them
    for f in ("ssl_version", "tls_cipher_suite", "tls_key_share"):
        m[f][clear] = 0
    m["tls_types"] = rng.choice(np.array([0, 0, 1, 2, 63, 0x40, 0xFF, 36], dtype=np.uint8), n)
    m["eth_protocol"][::5] = 0x86DD
    m["eth_protocol"][3::7] = 0x0800
    ids["src_ip"][3::7, 0] = 0x20
    ids["dst_ip"][3::7, 10] = 0x12
    m["eth_protocol"][6::11] = 0x0806
    ids["transport_protocol"] = rng.choice(np.array([1, 6, 6, 17, 58, 132, 47, 0], dtype=np.uint8), n)
    v6 = m["eth_protocol"] == 0x86DD
    sparse = (rng.integers(0, 3, (n, 16)) > 0) & (rng.integers(0, 2, (n, 1)) > 0)      # zero bytes: zero groups, short groups
    ids["src_ip"][v6] = (rng.integers(0, 256, (n, 16)) * sparse)[v6]
    ids["dst_ip"][v6] = (rng.integers(0, 256, (n, 16)) * sparse[:, ::-1])[v6]
    m["bytes"][::13] = 0
    m["bytes"][5::17] = 2**64 - 1
    m["packets"][::19] = 0
    m["packets"][7::23] = 2**32 - 1
    m["sampling"] = rng.choice(np.array([0, 0, 1, 50, 2**32 - 1], dtype=np.uint32), n)
    m["dscp"] = rng.choice(np.array([0, 8, 46, 255], dtype=np.uint8), n)
    m["start_mono_time_ts"][2::29] = 0
    m["end_mono_time_ts"][4::31] = 2**64 - 5                                           # ahead of the clock by a wrap
    m["start_mono_time_ts"][9::37] = 2**63 + 12345
    m["if_index_first_seen"][::6] = rng.integers(0, 10, len(m[::6]))
    worst = np.arange(n) % 41 == 11
    m["if_index_first_seen"][worst] = 7
    m["nb_observed_intf"][worst] = 6
    m["observed_intf"][worst] = 7
    m["src_mac"][::3] = np.frombuffer(bytes.fromhex("aabbccddeeff"), dtype=np.uint8)
    m["dst_mac"][::3] = np.frombuffer(bytes.fromhex("020000000002"), dtype=np.uint8)
    return recs


def check(got, want):
    buf, off, deferred = got
    wbuf, woff, wdef = want
    assert np.asarray(off).astype(np.uint64).tolist() == woff.tolist()
    assert np.asarray(deferred).tolist() == wdef.tolist()
    g = np.asarray(buf).tobytes()
    if g != wbuf:
        gl, wl = g.split(b"\n"), wbuf.split(b"\n")
        k = next(i for i, (a, b) in enumerate(zip(gl, wl)) if a != b)
        raise AssertionError("line %d:\n got %r\nwant %r" % (k, gl[k], wl[k]))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1025, 50_000])
def test_stream_parity_with_restatement(nf, O, n):
    recs = stream(nf, O, n, seed=n + 1)
    want = R.encode(recs, NOW, MONO, rows(NAMES), AGENT, RECEIVED)
    with nf.FlowTable(max_entries=64) as tab:
        got = tab.encode_flp_json(recs, NOW, MONO, table(nf, NAMES), AGENT, RECEIVED)
    assert not got[2].any(), "the parity streams clear the deferring fields: no record is left out"
    if n >= 1023:
        lens = np.diff(want[1].astype(np.int64))
        assert lens.max() > 3000 and lens.min() < 400            # worst-case and short lines side by side
    check(got, want)


def test_nil_agent_v6_agent_unknown_name_with_escapes_and_times_before_1970(nf, O):
    recs = stream(nf, O, 700, seed=77)
    with nf.FlowTable(max_entries=64) as tab:
        for agent, now, received, unknown in ((None, 5, -7, b'?"\n'), (bytes.fromhex("fd00000000000000000000000000000a"), -10**15, 0, b""),
                                              (bytes([192, 168, 0, 1]), NOW, 2**62, b"u" * 16)):
            want = R.encode(recs, now, MONO, rows(NAMES[:4]), agent, received, unknown)
            check(tab.encode_flp_json(recs, now, MONO, table(nf, NAMES[:4]), agent, received, unknown), want)


def test_deferred_records_are_flagged_and_the_rest_still_match(nf, O):
    """Variant 1 sets the TLS fields: kept here on every third record. The mask equals, record for record, the one computed
    from the input."""
    recs = stream(nf, O, 5000, seed=9, keep_tls=True)
    m = recs["metrics"]
    mask = ((m["ssl_version"] != 0) | (m["tls_cipher_suite"] != 0) | (m["tls_key_share"] != 0)).astype(np.uint8)
    assert 0 < mask.sum() < len(recs)
    want = R.encode(recs, NOW, MONO, rows(NAMES), AGENT, RECEIVED)
    assert want[2].tolist() == mask.tolist()
    with nf.FlowTable(max_entries=64) as tab:
        buf, off, deferred = tab.encode_flp_json(recs, NOW, MONO, table(nf, NAMES), AGENT, RECEIVED)
    assert deferred.tolist() == mask.tolist()
    lens = np.diff(off.astype(np.int64))
    assert (lens[mask == 1] == 0).all() and (lens[mask == 0] > 0).all()
    check((buf, off, deferred), want)


def test_namer_table_larger_than_lds(nf, O):
    """More rows than the size kernel stages in LDS (96): the lookups go to the table in HBM, same bytes."""
    names = [(1000 + k, None, "if%d" % k, "udn%d" % k if k % 3 else "") for k in range(150)] + NAMES
    recs = stream(nf, O, 3000, seed=8)
    recs["metrics"]["if_index_first_seen"][::2] = 1000 + (np.arange(1500) % 150)
    recs["metrics"]["observed_intf"][::4, 1] = 1000 + (np.arange(750) % 150)
    with nf.FlowTable(max_entries=64) as tab:
        check(tab.encode_flp_json(recs, NOW, MONO, table(nf, names), AGENT, RECEIVED, b"?"),
              R.encode(recs, NOW, MONO, rows(names), AGENT, RECEIVED, b"?"))
        check(tab.encode_flp_json(recs, NOW, MONO, table(nf, names[140:]), AGENT, RECEIVED, b"?"),
              R.encode(recs, NOW, MONO, rows(names[140:]), AGENT, RECEIVED, b"?"))


def test_truncated_then_written(nf, O):
    import torch
    recs = stream(nf, O, 300, seed=3, keep_tls=True)
    names = table(nf, NAMES)
    want, want_off, want_def = R.encode(recs, NOW, MONO, rows(NAMES), AGENT, RECEIVED)
    with nf.FlowTable(max_entries=64) as tab:
        # host entry point
        o, keep = nf.flp_options(NOW, MONO, names, AGENT, RECEIVED)
        need, n_def = C.c_size_t(0), C.c_size_t(0)
        small = np.full(len(want) - 1, 0xAB, dtype=np.uint8)
        off = np.zeros(301, dtype=np.uint64)
        flags = np.full(300, 0xCD, dtype=np.uint8)
        rc = nf._lib.lib.nfagg_encode_flp_json(tab._h, recs.ctypes.data_as(C.c_void_p), 300, C.byref(o), small.ctypes.data_as(C.c_void_p),
                                               len(small), off.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p), C.byref(n_def),
                                               C.byref(need))
        assert rc == nf.TRUNCATED and need.value == len(want) and n_def.value == int(want_def.sum())
        assert (small == 0xAB).all() and not off.any() and (flags == 0xCD).all()
        # device entry point: the first call says how much, writes nothing; the second writes it
        d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
        d_out = torch.full((len(want) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        d_off = torch.zeros(301, dtype=torch.int64, device="cuda")
        d_def = torch.full((300,), 0xCD, dtype=torch.uint8, device="cuda")
        rc, got, nd = tab.encode_flp_json_device(d_recs.data_ptr(), 300, NOW, MONO, names, AGENT, RECEIVED, d_out.data_ptr(), len(want) - 1,
                                                 d_off.data_ptr(), d_def.data_ptr())
        torch.cuda.synchronize()
        assert rc == nf.TRUNCATED and got == len(want) and nd == int(want_def.sum())
        assert (d_out.cpu().numpy() == 0xAB).all() and not d_off.cpu().numpy().any() and (d_def.cpu().numpy() == 0xCD).all()
        rc, got, nd = tab.encode_flp_json_device(d_recs.data_ptr(), 300, NOW, MONO, names, AGENT, RECEIVED, 0, 1 << 30, d_off.data_ptr())
        assert rc == nf.TRUNCATED and got == len(want) and not d_off.cpu().numpy().any()          # d_out == NULL: the size
        rc, got, nd = tab.encode_flp_json_device(d_recs.data_ptr(), 300, NOW, MONO, names, AGENT, RECEIVED, d_out.data_ptr(), len(want),
                                                 d_off.data_ptr(), d_def.data_ptr())
        torch.cuda.synchronize()
        assert rc == nf.OK and got == len(want) and nd == int(want_def.sum())
        out = d_out.cpu().numpy()
        assert (out[len(want):] == 0xAB).all()
        check((out[: len(want)], d_off.cpu().numpy(), d_def.cpu().numpy()), (want, want_off, want_def))


def test_chained_calls_equal_one_call(nf, O):
    recs = stream(nf, O, 5000, seed=4)
    names = table(nf, NAMES)
    with nf.FlowTable(max_entries=64) as tab:
        whole, off, _ = tab.encode_flp_json(recs, NOW, MONO, names, AGENT, RECEIVED)
        a, off_a, _ = tab.encode_flp_json(recs[:3333], NOW, MONO, names, AGENT, RECEIVED)
        b, off_b, _ = tab.encode_flp_json(recs[3333:], NOW, MONO, names, AGENT, RECEIVED)
    assert a.tobytes() + b.tobytes() == whole.tobytes()
    assert off_a.tolist() + (off_b[1:] + off_a[-1]).tolist() == off.tolist()


def _clear_tls_on_two_of_three(torch, d_ev, n):
    """Variant 1 sets the TLS fields on every flow, which would defer them all: zero ssl_version / tls_cipher_suite /
    tls_key_share (record bytes 132..137) of the evicted records in HBM, except on every third one."""
    v = d_ev[: n * 144].view(n, 144)
    v[torch.arange(n, device="cuda") % 3 != 0, 132:138] = 0
    torch.cuda.synchronize()


def test_device_resident_evict_then_encode(nf, O):
    """nfagg_evict_device -> nfagg_encode_flp_json_device without leaving HBM, against the restatement on the host copy."""
    import torch
    th = O.zipf_thresholds(3000, 1.1)
    recs = O.gen_stream(100_000, seed=12, n_keys=3000, thresholds=th, variant=1)
    recs["metrics"]["eth_protocol"][::5] = 0x86DD
    names = table(nf, NAMES)
    with nf.FlowTable(max_entries=1 << 16) as tab:
        assert tab.ingest(recs.view(nf.FLOW_RECORD)) == (nf.OK, len(recs))
        d_ev = torch.empty(3000 * 144 + 16, dtype=torch.uint8, device="cuda")
        n = tab.evict_device(d_ev.data_ptr(), 3000)
        assert 0 < n <= 3000
        _clear_tls_on_two_of_three(torch, d_ev, n)
        d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_def = torch.empty(n, dtype=torch.uint8, device="cuda")
        rc, need, nd = tab.encode_flp_json_device(d_ev.data_ptr(), n, NOW, MONO, names, AGENT, RECEIVED, 0, 0, d_off.data_ptr())
        assert rc == nf.TRUNCATED and need > 0                   # size query
        d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
        rc, wrote, nd = tab.encode_flp_json_device(d_ev.data_ptr(), n, NOW, MONO, names, AGENT, RECEIVED, d_out.data_ptr(), need,
                                                   d_off.data_ptr(), d_def.data_ptr())
        assert rc == nf.OK and wrote == need
        ev = d_ev[: n * 144].cpu().numpy().view(nf.FLOW_RECORD)
        got = (d_out[:need].cpu().numpy(), d_off.cpu().numpy(), d_def.cpu().numpy())
    want = R.encode(ev, NOW, MONO, rows(NAMES), AGENT, RECEIVED)
    assert nd == int(want[2].sum()) and 0 < nd < len(ev) / 2
    check(got, want)


def test_one_million_flows_evicted_and_encoded_on_the_device(nf, O):
    import torch
    from netobserv_ebpf_agent_amd import synth
    flows, n = 1_000_000, 8_000_000
    d_th = torch.from_numpy(synth.zipf_thresholds(flows, 1.1).view(np.int64)).cuda()
    d = torch.empty(n * 144, dtype=torch.uint8, device="cuda")
    synth.stream_device(d.data_ptr(), n, seed=2, n_keys=flows, d_thresholds=d_th.data_ptr(), variant=1)
    names = table(nf, NAMES)
    with nf.FlowTable(max_entries=1 << 21) as tab:
        assert tab.ingest_device(d.data_ptr(), n) == (nf.OK, n)
        d_ev = torch.empty(flows * 144 + 16, dtype=torch.uint8, device="cuda")
        m = tab.evict_device(d_ev.data_ptr(), flows)
        assert m > 500_000
        _clear_tls_on_two_of_three(torch, d_ev, m)
        d_off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
        d_def = torch.empty(m, dtype=torch.uint8, device="cuda")
        rc, need, nd = tab.encode_flp_json_device(d_ev.data_ptr(), m, NOW, MONO, names, AGENT, RECEIVED, 0, 0, d_off.data_ptr())
        d_out = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
        rc, wrote, nd = tab.encode_flp_json_device(d_ev.data_ptr(), m, NOW, MONO, names, AGENT, RECEIVED, d_out.data_ptr(), need,
                                                   d_off.data_ptr(), d_def.data_ptr())
        assert rc == nf.OK and wrote == need
        ev = d_ev[: m * 144].cpu().numpy().view(nf.FLOW_RECORD)
        got = (d_out[:need].cpu().numpy(), d_off.cpu().numpy(), d_def.cpu().numpy())
    want = R.encode(ev, NOW, MONO, rows(NAMES), AGENT, RECEIVED)
    assert nd == int(want[2].sum()) and 0 < nd < len(ev) / 2
    check(got, want)


def test_c_driver_matches_restatement(nf, O, tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "netobserv-ebpf-agent_amd", "lib")
    exe = str(tmp_path / "nfagg_flp_cdriver")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tools", "c", "nfagg_flp_cdriver.c"), "-o", exe, "-L", libdir, "-lnfagg", "-Wl,-rpath," + libdir])
    recs = stream(nf, O, 2000, seed=11, keep_tls=True)
    recs["metrics"]["if_index_first_seen"][::4] = 3
    (tmp_path / "in.bin").write_bytes(recs.tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "in.bin"), str(tmp_path / "o"), str(NOW), str(MONO), str(RECEIVED)], text=True, timeout=120)
    names = [(2, None, b"eth0", b""), (3, bytes.fromhex("020000000001"), b"veth3a", b"blue"), (3, None, b"veth3", b"")]
    want, want_off, want_def = R.encode(recs, NOW, MONO, names, bytes(10) + b"\xff\xff" + bytes([10, 9, 8, 7]), RECEIVED)
    assert out.split() == ["lines", "2000", "deferred", str(int(want_def.sum())), "bytes", str(len(want))]
    assert (tmp_path / "o.json").read_bytes() == want
    assert np.fromfile(tmp_path / "o.off", dtype=np.uint64).tolist() == want_off.tolist()
    assert np.fromfile(tmp_path / "o.def", dtype=np.uint8).tolist() == want_def.tolist()


def test_config0_end_to_end_same_lines_as_direct_flp_stdout(nf, O):
    """configs[0]: ring records -> Accounter.Account (libnfagg) -> CapacityLimiter.Limit -> StartDirectFLPJSON gives the same set
    of lines as DirectFLPStdout on the same run."""
    from netobserv_ebpf_agent_amd import accounter as A
    names = {2: "eth0", 3: "eth1", 4: "br-ex", 5: "ovn-k8s-mp0"}
    now, mono = 1_700_000_000_000_000_000, 3_000_000
    recs = O.gen_stream(10_000, seed=1, n_keys=1_000)
    namer, ip = A._interface_namer, A._agent_ip
    nf.SetInterfaceNamer(lambda ifx, mac: names.get(ifx, "unknown")); nf.SetGlobalIP(ipaddress.ip_address("10.1.2.3"))
    try:
        acc = nf.NewAccounter(1 << 16, 3600.0, lambda: now, lambda: mono)
        q_in, q_mid, q_out = queue.Queue(), queue.Queue(), queue.Queue(maxsize=50)
        limiter = nf.CapacityLimiter(nf.NoOp())

        def forward():                                    # Account() returns after the closing eviction; Go closes the channel
            t = threading.Thread(target=limiter.Limit, args=(q_mid, q_out))
            t.start()
            acc_thread.join()
            q_mid.put(nf.CLOSE)
            t.join()

        batches = []

        def collect():
            while True:
                b = q_out.get()
                if b is nf.CLOSE:
                    return
                batches.append(b)

        acc_thread = threading.Thread(target=acc.Account, args=(q_in, q_mid))
        threads = [acc_thread, threading.Thread(target=forward), threading.Thread(target=collect)]
        for t in threads:
            t.start()
        for off in range(0, 10_000, 1000):
            q_in.put(recs[off:off + 1000].view(nf.FLOW_RECORD))
        q_in.put(nf.CLOSE)
        for t in threads:
            t.join(timeout=60)
            assert not t.is_alive()
        acc.close()
        text, q = io.StringIO(), queue.Queue()
        for b in batches:
            q.put(b)
        q.put(nf.CLOSE)
        nf.DirectFLPStdout(text, time_received=RECEIVED).ExportFlows(q)
        # the same batches through the GPU exporter: the records the Accounter evicted, raw
        out = io.BytesIO()
        with nf.FlowTable(max_entries=64) as tab:
            exp = nf.StartDirectFLPJSON(tab, out, names=nf.intf_table([(i, None, n, "") for i, n in names.items()]),
                                        agent_ip=ipaddress.ip_address("10.1.2.3").packed, time_received=lambda: RECEIVED)
            q = queue.Queue()
            for b in batches:
                raw = np.zeros(len(b), dtype=nf.FLOW_RECORD)
                for k, rec in enumerate(b):
                    raw[k]["id"], raw[k]["metrics"] = rec.ID, rec.Metrics
                q.put((raw, now, mono))
            q.put(nf.CLOSE)
            exp.ExportFlows(q)
    finally:
        nf.SetInterfaceNamer(namer); nf.SetGlobalIP(ip)
    want = sorted(text.getvalue().encode().splitlines())
    assert len(want) > 990 and exp.deferred == 0
    assert sorted(out.getvalue().splitlines()) == want
