"""Every object of the library frees what it allocated (csrc/nfagg_handle.h: the owner types): nfagg_debug_live_buffers counts
the device and page-locked allocations of the library that are alive in the process, and creating, using and closing one of
everything brings it back to where it was. The count is the library's own, so other tenants of the GPU do not move it."""
import numpy as np
import pytest

import conn_cases as CC

pytestmark = pytest.mark.gpu

MAX_ENTRIES = 5000                       # 2^16 slots, the smallest table
PAR_MIN = 31_049                         # account_par_min_records(5000) (csrc/nfagg_api_account.hip)
NOW, MONO = 1_700_000_000_123_456_789, 2_500_000
AGENT = bytes(range(16))
CYCLES = 6


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def streams(nf, O):
    """The inputs of every cycle, made once: [0] the first call's, [1] the larger second call's."""
    rng = np.random.default_rng(7)
    recs = O.gen_stream(40_000, seed=21, n_keys=20_000, variant=1).view(nf.FLOW_RECORD)

    def maps(n, n_cpu):
        ids = np.zeros(n, dtype=nf.FLOW_ID)
        ids.view(np.uint8).reshape(n, 40)[:] = rng.integers(0, 256, (n, 40), dtype=np.uint8)
        vals = np.zeros(n, dtype=nf.FLOW_METRICS)
        vals.view(np.uint8).reshape(n, 104)[:] = rng.integers(0, 256, (n, 104), dtype=np.uint8)
        dt = nf.ROLLUP_KINDS["dns"]
        parts = np.zeros(n * n_cpu, dtype=dt)
        parts.view(np.uint8)[:] = rng.integers(0, 256, parts.nbytes, dtype=np.uint8)
        return ids, vals, parts

    return dict(recs=recs, maps=[maps(50, 2), maps(3000, 2)], names=nf.intf_table([(2, None, "eth0", ""), (3, None, "eth1", "default")]))


def dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()             # the upload runs on torch's stream, the library's calls on its own
    return t


def use_table(nf, torch, tab, S, second):
    """Every scratch family of an accounter-mode table once; second: the same calls with larger inputs that take the same paths
    (a host ingest of more records than the table holds, say, would be folded optimistically and snapshot the sketches: a
    buffer of its own, not one that grew)."""
    recs = S["recs"]
    n_small, n_enc, n_par = (4000, 3000, PAR_MIN + 4000) if second else (2000, 300, PAR_MIN + 150)
    tab.ingest(recs[:n_small])                                   # the staging ring, the spill queues or the careful path
    assert len(tab.evict()) > 0                                  # the eviction buffer, the bounce path
    d = dev(torch, recs[:n_par])
    out = torch.empty((n_par + MAX_ENTRIES) * 144 + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    first = tab.stats().account_epochs_first
    rc, consumed, ends = tab.account_device(d.data_ptr(), n_par, out.data_ptr(), n_par + MAX_ENTRIES, 64)
    assert rc == nf.OK and consumed == n_par and len(ends) >= 1
    assert tab.stats().account_epochs_first == first + 1         # the epochs-found-first path took it
    tab.evict()
    ids, vals, parts = S["maps"][second]
    tab.rollup("dns", parts, 2, vals)
    merged = tab.map_merge(ids, vals, {"dns": (ids, parts)}, 2)
    assert len(merged[0]) == len(ids)
    tab.ingest(recs[:n_enc])
    assert len(tab.cm_topk(nf.CM_SRC, recs[:n_enc], 5)) == 5
    assert len(tab.encode_pb(recs[:n_enc], NOW, MONO, AGENT, S["names"])[1]) == n_enc + 1
    assert len(tab.encode_ipfix(recs[:n_enc], NOW, MONO, S["names"], 1_700_000_000, 0)[1]) == n_enc + 1
    assert len(tab.encode_flp_json(recs[:n_enc], NOW, MONO, S["names"], AGENT)[1]) == n_enc + 1
    buf = torch.zeros(MAX_ENTRIES * tab.partial_bytes + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, counts, total = tab.partials_export_device(2, 0xFFFFFFFF, buf.data_ptr(), MAX_ENTRIES)      # NFAGG_SHARD_NONE: a count, a scatter
    assert rc == nf.OK and sum(counts) == total > 0
    tab.evict()


def one_cycle(nf, torch, S, grow):
    recs = S["recs"]
    with nf.FlowTable(max_entries=MAX_ENTRIES, staging_records=1, sketches=nf.SKETCH_CM | nf.SKETCH_HLL, cm_log2_width=10, hll_p=8) as tab, \
            nf.FlowTable(max_entries=MAX_ENTRIES, staging_records=1, ingest_variant=30) as chain, \
            nf.FlowTable(max_entries=MAX_ENTRIES, staging_records=1, mode=nf.MODE_KERNEL_DEDUP, local_fold=True) as sub:
        with nf.NetevTable([], table=tab), nf.TlsNames(table=tab), nf.K8sTable([], table=tab) as k8s, nf.NetTable(0, table=tab) as net, \
                nf.MetricsTable(k8s, [nf.metrics.KEY_DIMS["SrcK8S_Name"]], table=tab), nf.ConnLayout(CC.FIELDS_COUNT, table=tab), \
                nf.Filter(nf.TransformFilter(None), k8s, net, table=tab):
            use_table(nf, torch, tab, S, False)
            if grow:
                before = nf.debug_live_buffers()
                use_table(nf, torch, tab, S, True)
                assert nf.debug_live_buffers() == before, "a scratch buffer that grew must replace its block, not add one"
        # the kernel chain: from host memory in one-record chunks (the control block's mirror, both eviction buffers), then device-resident
        chained = chain.stats().account_chain
        rc, consumed, _ = chain.account(recs[:40])
        assert rc == nf.OK and consumed == 40
        d = dev(torch, recs[:12_000])
        out = torch.empty((12_000 + MAX_ENTRIES) * 144 + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc, consumed, ends = chain.account_device(d.data_ptr(), 12_000, out.data_ptr(), 12_000 + MAX_ENTRIES, 16)
        assert rc == nf.OK and consumed == 12_000 and chain.stats().account_chain > chained
        # the sub-flow table: the aux lines from the start, the join table at the first eviction
        sub.ingest_device(d.data_ptr(), 4000)
        assert len(sub.evict()) > 0
    with nf.FlowGroup([0, 0], max_entries=MAX_ENTRIES, staging_records=4096) as grp:
        grp.ingest(recs[:3000])
        assert len(grp.evict()) > 0


def test_every_object_returns_the_buffers_it_took(nf, O, torch, streams):
    live = nf.debug_live_buffers
    start = live()
    for cycle in range(CYCLES):
        one_cycle(nf, torch, streams, grow=cycle == 1)
        assert live() == start, f"cycle {cycle}: {live() - start} allocations outlive their owners"


def test_a_create_that_fails_its_checks_allocates_nothing(nf):
    start = nf.debug_live_buffers()
    with pytest.raises(nf.NfaggError):
        nf.FlowTable(max_entries=1 << 20, table_log2_slots=16)   # 2^16 slots < 2 * max_entries
    assert nf.debug_live_buffers() == start
