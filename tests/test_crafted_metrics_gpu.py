"""The metrics fold (csrc/nfagg_metrics.hip) on CRAFTED group hashes. tests/test_flp_metrics_gpu.py covers sizes, overflow and
groups that share their first key half, but nothing there makes groups share a HOME SLOT: the LDS probe window overflowing into
the direct global path, probe chains that wrap round the end of the LDS and the global table, and two keys with one first half
meeting in one slot (the half-claimed-slot rule of the claim protocol) are reached by luck or not at all. A group's key is made of
small fields, so keys cannot be solved for — but 600 rows x 600 rows x 8 protocols are 2.88 M candidate keys under the grouping
"src name, dst name, proto", and brute force over them with the pinned restatement of the hash (keycraft.metrics_group_hash,
tests/test_crafted_sketches_cpu.py) is instant:

    lds_one_home      64 groups with one LDS home slot; cap 512, so the global table has as many slots as the LDS one: the first
                      kMetLdsProbe of them fill the probe window, the others take the direct global path, one chain of 64 there
    wrap              40 groups whose homes are the last three slots of the 1 024-slot tables (LDS and global wrap together);
                      30 on the last three slots of an 8 192-slot global table (cap 4 096)
    same_first_half   200 (src, dst) pairs of which two protocols share an LDS home, and every pair of which three do: one first
                      key half, two second halves, one slot; whole waves of A, B, A, B ..., twice, so that both keys are hot in
                      one workgroup and two workgroups flush them into one global slot
    low32             200 pairs of groups with equal low 32 hash bits: one home in every table; caps 512 and 65 536
    exact_cap         the ~39 500 groups of test_flp_metrics_gpu's `large` stream against a cap of exactly their number (ten
                      workgroups' flushes race on the claim counter up to the cap itself), and of one less

Expected: check_fold / numpy_groups of tests/test_flp_metrics_gpu.py, unchanged, on the host and device entry points. Each family's
precondition is computed from the groups the DEVICE returned, through the library's exported hash."""
import numpy as np
import pytest

import flp_json_net_ref as R
import keycraft as kc
import test_flp_metrics_gpu as MG
from test_flp_metrics_gpu import large, tab  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROWS, BACKGROUND_ROWS = 600, 7
PROTOS = np.array([6, 17, 1, 58, 132, 47, 50, 51])
CONSTS = kc.metrics_constants()
LDS = CONSTS["kMetLdsSlots"]


class World:
    def __init__(self, nf):
        self.nf = nf
        self.addr = np.zeros((ROWS, 16), dtype=np.uint8)
        self.addr[:, 10:12], self.addr[:, 12], self.addr[:, 13], self.addr[:, 14], self.addr[:, 15] = 0xFF, 10, 77, np.arange(ROWS) >> 8, np.arange(ROWS) & 255
        self.entries = [(self.addr[k].tobytes(), dict(namespace="ns-%d" % (k % 50), name="obj-%d" % k, kind="Pod")) for k in range(ROWS)]
        self.dims = MG.dims_of(nf, "SrcK8S_Name", "DstK8S_Name", "Proto")
        # distinct names: row k is class k + 1 on either side (check_fold verifies the classes of what comes back)
        i, j, q = np.meshgrid(np.arange(ROWS), np.arange(ROWS), np.arange(len(PROTOS)), indexing="ij")
        self.hash = kc.metrics_group_hash(0, i + 1, j + 1, proto=PROTOS[q], is_ip=1)     # (600, 600, 8)

    def groups(self, flat):
        """Flat candidate indexes -> (k, 3) of (src row, dst row, protocol)."""
        i, j, q = np.unravel_index(np.asarray(flat), self.hash.shape)
        return np.stack([i, j, PROTOS[q]], axis=1)

    def records(self, ijp, rng):
        ijp = np.asarray(ijp)
        recs = np.zeros(len(ijp), dtype=self.nf.FLOW_RECORD)
        recs["id"]["src_ip"], recs["id"]["dst_ip"] = self.addr[ijp[:, 0]], self.addr[ijp[:, 1]]
        recs["metrics"]["eth_protocol"], recs["id"]["transport_protocol"] = 0x0800, ijp[:, 2]
        recs["metrics"]["bytes"], recs["metrics"]["packets"] = rng.integers(0, 2**40, len(ijp)), rng.integers(0, 100, len(ijp))
        return recs

    def background(self, n, rng):
        return np.stack([rng.integers(0, BACKGROUND_ROWS, n), rng.integers(0, BACKGROUND_ROWS, n), np.full(n, 6)], axis=1)

    def scattered(self, planted, rng, reps=40):
        """Every planted group `reps` times among background flows, shuffled: every workgroup meets every planted group."""
        n = max(5 * CONSTS["kMetFlowsPerBlock"] + 777, reps * len(planted) + 4000)
        ijp = np.concatenate([np.repeat(planted, reps, axis=0), self.background(n - reps * len(planted), rng)])
        return self.records(ijp[rng.permutation(len(ijp))], rng)

    def fold(self, tab, recs, cap):
        got = MG.check_fold(self.nf, tab, self.entries, None, R.RULES_OFF, [self.dims], recs, caps=[cap])[0]
        assert len(recs) > 4 * CONSTS["kMetFlowsPerBlock"], "at least five workgroups"
        return got, self.nf.metrics_group_hash(0, got)


@pytest.fixture(scope="module")
def world(nf):
    return World(nf)


def test_restatement_agrees_with_the_library_on_the_candidates(nf, world):
    rng = np.random.default_rng(1)
    flat = rng.integers(0, world.hash.size, 2000)
    g = np.zeros(len(flat), dtype=nf.METRIC_GROUP)
    ijp = world.groups(flat)
    g["src_class"], g["dst_class"], g["proto"], g["is_ip"] = ijp[:, 0] + 1, ijp[:, 1] + 1, ijp[:, 2], 1
    g["src_label"], g["dst_label"], g["direction"] = nf._lib.NET_NO_LABEL, nf._lib.NET_NO_LABEL, nf._lib.NET_NO_DIRECTION
    assert np.array_equal(nf.metrics_group_hash(0, g), world.hash.ravel()[flat])


def test_lds_one_home(nf, tab, world):
    rng = np.random.default_rng(2)
    home = world.hash.ravel() & np.uint64(LDS - 1)
    planted = world.groups(np.flatnonzero(home == np.bincount(home.astype(np.int64)).argmax())[:64])
    got, h = world.fold(tab, world.scattered(planted, rng), 512)
    assert 2 * 512 == LDS == CONSTS["kMetMinSlots"], "the family wants a global table with the LDS table's mask"
    most = int(np.bincount((h & np.uint64(LDS - 1)).astype(np.int64)).max())
    print("lds_one_home: %d groups, %d share one LDS home (precondition: >= 64 > kMetLdsProbe = %d)" % (len(got), most, CONSTS["kMetLdsProbe"]))
    assert most >= 64 > CONSTS["kMetLdsProbe"]


@pytest.mark.parametrize("cap,n_planted", [(512, 40), (4096, 30)])
def test_wrap(nf, tab, world, cap, n_planted):
    rng = np.random.default_rng(3)
    slots = max(2 * cap, CONSTS["kMetMinSlots"])
    last3 = lambda h: ((h & np.uint64(0xFFFFFFFF)) & np.uint64(slots - 1)) >= np.uint64(slots - 3)
    planted = world.groups(np.flatnonzero(last3(world.hash.ravel()))[:n_planted])
    got, h = world.fold(tab, world.scattered(planted, rng), cap)
    n_last = int(last3(h).sum())
    n_lds = int(((h & np.uint64(LDS - 1)) >= np.uint64(LDS - 3)).sum())
    print("wrap: %d groups; %d with a home in the last three of %d slots (precondition: >= %d); %d in the last three LDS slots" % (len(got), n_last, slots, n_planted, n_lds))
    assert n_last >= n_planted > 3 + CONSTS["kMetLdsProbe"]
    assert slots != LDS or n_lds >= n_planted


def same_home_protocols(world):
    """(pairs, triples): per (src, dst) the protocol indexes that share an LDS home — exactly two of the eight, or three."""
    home = world.hash & np.uint64(LDS - 1)
    nq = len(PROTOS)
    pairs, triples = {}, {}
    for a in range(nq):
        for b in range(a + 1, nq):
            eq = home[:, :, a] == home[:, :, b]
            for i, j in zip(*np.nonzero(eq)):
                pairs.setdefault((int(i), int(j)), set()).update((a, b))
    for key in [k for k, v in pairs.items() if len(v) >= 3]:
        v = sorted(pairs.pop(key))
        if len(v) == 3 and len({int(home[key[0], key[1], q]) for q in v}) == 1:
            triples[key] = v
    return {k: sorted(v) for k, v in pairs.items()}, triples


def test_same_first_half(nf, tab, world):
    rng = np.random.default_rng(4)
    pairs, triples = same_home_protocols(world)
    assert len(pairs) >= 200 and len(triples) >= 1
    chosen = [(k, pairs[k]) for k in sorted(pairs)[:200]] + [(k, triples[k]) for k in sorted(triples)]
    waves = []
    for (i, j), qs in chosen:                                                             # one wave of 64 records per pair: A, B, A, B, ...
        waves.append(np.array([[i, j, PROTOS[qs[k % len(qs)]]] for k in range(64)]))
    block = np.concatenate(waves)
    n_bg = max(0, 5 * CONSTS["kMetFlowsPerBlock"] + 777 - 2 * len(block)) + 3000
    recs = world.records(np.concatenate([block, world.background(n_bg, rng), block]), rng)
    assert 2 * len(chosen) + len(triples) + BACKGROUND_ROWS**2 <= 512
    got, h = world.fold(tab, recs, 512)                                                  # 1 024 global slots: LDS home == global home
    per = {}
    for g, x in zip(got, (h & np.uint64(LDS - 1)).tolist()):
        per.setdefault((int(g["src_class"]), int(g["dst_class"]), x), []).append(int(g["proto"]))
    two, three = sum(1 for v in per.values() if len(v) == 2), sum(1 for v in per.values() if len(v) >= 3)
    print("same_first_half: %d groups; %d (src, dst) pairs with two protocols on one LDS home, %d with three (preconditions: >= 200, == %d)" % (len(got), two, three, len(triples)))
    assert two >= 200 and three == len(triples)
    keys = {(i + 1, j + 1, int(PROTOS[q])) for (i, j), qs in chosen for q in qs}
    hot = [int(g["flows"]) for g in got if (int(g["src_class"]), int(g["dst_class"]), int(g["proto"])) in keys]
    assert len(hot) == len(keys) and min(hot) >= 2 * 21                                   # every planted key is hot in its waves


@pytest.mark.parametrize("cap", [512, 65536])
def test_low32(nf, tab, world, cap):
    rng = np.random.default_rng(5)
    low = (world.hash.ravel() & np.uint64(0xFFFFFFFF))
    order = np.argsort(low, kind="stable")
    s = low[order]
    eq = np.flatnonzero(s[1:] == s[:-1])
    eq = eq[np.concatenate([[True], np.diff(eq) > 1])][:200]                              # disjoint pairs
    planted = world.groups(np.concatenate([order[eq], order[eq + 1]]))
    got, h = world.fold(tab, world.scattered(planted, rng, reps=30), cap)
    l32, counts = np.unique(h & np.uint64(0xFFFFFFFF), return_counts=True)
    print("low32: %d groups, %d pairs with equal low 32 hash bits (precondition: >= 200), cap %d" % (len(got), int((counts >= 2).sum()), cap))
    assert int((counts >= 2).sum()) >= 200 and len(np.unique(h)) == len(h)


def test_exact_cap(nf, tab, large):
    """A cap of exactly the number of groups: NFAGG_OK and the exact groups, with the ten workgroups' flushes racing on the claim
    counter; one less: NFAGG_TRUNCATED, a count above the cap, nothing written (fold_both's canaries cover the outputs)."""
    recs, entries = large
    dims = MG.dims_of(nf, "SrcK8S_Name", "DstK8S_Name")
    with tab.k8s_table(entries) as k8s, tab.metrics_table(k8s, [dims]) as met:
        k8s_rows = tab.k8s_resolve(k8s, recs)
        want = MG.by_key(MG.numpy_groups(nf, dims, entries, None, recs, k8s_rows, None))
        n = len(want)
        assert 39_000 < n <= 40_000
        rc, got, counts = MG.fold_both(nf, tab, met, recs, k8s_rows, None, [n])
        assert rc == nf.OK and counts == [n] and got[0].tobytes() == want.tobytes()
        rc, got, counts = MG.fold_both(nf, tab, met, recs, k8s_rows, None, [n - 1])
        assert rc == nf.TRUNCATED and counts[0] > n - 1 and len(got[0]) == 0
