"""The stable partition of the routed group (csrc/nfagg_partition.hip) past its own thresholds. It partitions a whole
nfagg_group_ingest_device call at once; the largest routed call elsewhere in the suite is 500 000 records — 123 tiles — so
k_part_scan's running total never left its first chunk of tiles, k_part_count and k_part_scatter never walked a second tile per
workgroup, and no group had more than 8 members of the 64 the kernels' LDS arrays are sized for. The thresholds are in tiles, so
the streams are millions of records, generated on the device; the sizes are read from the source (keycraft.partition_constants).

Expected, always: every member evicts exactly the oracle's flows whose shard (keycraft.shard_formula, in Python integers) it is,
bit for bit — a record scattered to the wrong bucket, or out of arrival order inside its bucket, changes a flow — and the union is
the oracle's single Accounter over the host-generated stream."""
import numpy as np
import pytest

import keycraft as kc
from conftest import assert_records_equal
from test_device_path_gpu import dev_stream, torch  # noqa: F401  (torch: fixture)

pytestmark = pytest.mark.gpu

PC = kc.partition_constants()
TILE, SCAN_CHUNK, GRID_CAP = PC["tile"], PC["scan_chunk"], PC["grid_cap"]


def routed_call(nf, O, torch, n, n_members, keys, max_entries, seed, hot_permille=0, **group_kw):
    th = nf.synth.zipf_thresholds(keys, 1.1)
    d = dev_stream(torch, nf.synth, n, seed=seed, n_keys=keys, thresholds=th, variant=1, hot_permille=hot_permille)
    host = O.gen_stream(n, seed=seed, n_keys=keys, thresholds=th, variant=1, hot_permille=hot_permille)
    want = O.run_accounter(host, 1 << 20)
    assert len(want) == 1
    want = want[0][1]
    owner = kc.shard_formula(want, n_members)
    with nf.FlowGroup([0] * n_members, max_entries=max_entries, **group_kw) as grp:
        assert grp.ingest_device(0, d.data_ptr(), n) == (nf.OK, n)                       # ONE call: one partition of n records
        per_member = [int(m.stats().records_ingested) for m in grp.members]
        assert sum(per_member) == n and len(grp) == len(want)
        outs = [torch.empty((int((owner == j).sum()) + 1) * 144, dtype=torch.uint8, device="cuda") for j in range(n_members)]
        counts = grp.evict_device([o.data_ptr() for o in outs], [int((owner == j).sum()) + 1 for j in range(n_members)], nf.REASON_CLOSING)
    parts = []
    for j in range(n_members):
        got = nf.sort_by_key(outs[j][:counts[j] * 144].cpu().numpy().view(nf.FLOW_RECORD))
        assert_records_equal(got, want[owner == j], "member %d of %d" % (j, n_members))
        parts.append(got)
    assert_records_equal(nf.sort_by_key(np.concatenate(parts)), want, "the union")
    return per_member


@pytest.mark.parametrize("which", ["grid stride", "scan carry"])
def test_large_routed_call(nf, O, torch, which):
    """grid stride: grid cap x tile + 777 records (8 389 385 = 2 049 tiles, the last one ragged): the first workgroup of
    k_part_count / k_part_scatter walks a second tile, and k_part_scan carries its total over two chunk borders.
    scan carry: scan chunk x tile + 1 records (4 194 305 = 1 025 tiles): one tile of one record behind the first chunk, placed
    by nothing but the carry."""
    n = GRID_CAP * TILE + 777 if which == "grid stride" else SCAN_CHUNK * TILE + 1
    assert (n + TILE - 1) // TILE == (GRID_CAP + 1 if which == "grid stride" else SCAN_CHUNK + 1) and n < 1 << 31
    per_member = routed_call(nf, O, torch, n, 3, keys=30_000, max_entries=1 << 20, seed=61, hot_permille=300)
    assert min(per_member) > n // 20


@pytest.mark.parametrize("n_members", [33, 64])
def test_many_members(nf, O, torch, n_members):
    """More members than a wave has half its lanes, and kMaxShards itself: the per-shard ballots, the LDS histograms and the bucket
    bases of all 64 shards; three tiles and a ragged fourth."""
    assert n_members <= PC["kMaxShards"] == 64
    per_member = routed_call(nf, O, torch, 3 * TILE + 5, n_members, keys=3_000, max_entries=1 << 15, seed=62, staging_records=4096)
    assert min(per_member) > 0
