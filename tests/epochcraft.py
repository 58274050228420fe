"""Account calls built from a PLAN (a helper module, no fixtures): the flow of every record is chosen, so the evict-on-full loop of
Accounter.Account (pkg/flow/account.go:81-96) cuts exactly where the plan says, a flow's segment of an epoch has exactly the asked
number of records and sorted positions, and a chosen record of a segment carries the only non-zero DSCP. The seeded Zipf streams
of the other account tests put all of that wherever chance does.

The rule that makes a plan exact (tests/test_epoch_boundaries.py pins it):
    an epoch [c_t, c_t+1) holds exactly max_entries first occurrences (heads): one at c_t, the others wherever the plan puts them;
    every other record of the epoch repeats a flow the epoch has seen already;
    the record at c_t+1 is a flow that is NOT in the ending epoch: a fresh one, or a flow of an epoch before that one;
    a head may re-use a flow of the epoch directly before (its previous occurrence is >= 0 but below the epoch's start: "new"
    by comparison with the start, not by prev == -1); cuts are at least max_entries apart; with live0 flows in the table the
    first cut needs max_entries - live0 new flows before it (the table's flows are not new in the first epoch).

Keys are the distinct keys of a variant-1 stream of the oracle; the order-dependent fields of every record are that variant's
scramble. Flows that must share their 64-bit key hash, or sit in a chosen home slot, get their keys from keycraft.craft.
tests/test_epochcraft_cpu.py checks every call of cases() against the cut rule, the oracle and the numpy model of the segment folds;
tests/test_crafted_epochs_gpu.py runs them through the kernels."""
import zlib

import numpy as np

import keycraft as kc

M64 = (1 << 64) - 1
ORDER_FIELDS = ("eth_protocol", "dscp", "sampling", "src_mac", "dst_mac", "start", "end")


# ---------------------------------------------------------------- the sizes the plans are built around, read from the source
def constants():
    """Segment thresholds, the cut walk's geometry, the link search's bound and the chain's block and window, parsed from csrc/
    as keycraft.fold_constants does (a changed constant moves the tests with it). The row of 256 and the group of four records
    per lane are what cut_load's one 16-byte load per lane and row makes of a wave of 64 lanes."""
    par, chain = "nfagg_epoch_par.hip", "nfagg_epoch_chain.hip"
    c = {"S": kc._grab(par, r"^#define NF_SEG_SHORT (\d+)"), "H": kc._grab(par, r"^#define NF_SEG_HUGE (\d+)"),
         "C": kc._grab(par, r"^#define NF_HUGE_CHUNK (\d+)"), "kCutBlock": kc._grab(par, r"^constexpr int kCutBlock = (\d+);"),
         "kCutPer": kc._grab(par, r"^constexpr int kCutPer = (\d+);"), "kLinkSearch": kc._grab(par, r"^constexpr int kLinkSearch = (\d+);"),
         "kCkBlock": kc._grab(chain, r"^constexpr int kCkBlock = (\d+)"), "kCkGrid": kc._grab(chain, r"\bkCkGrid = (\d+);")}
    c["group"] = 4                                                    # records per lane and row (one int4)
    c["row"] = 64 * c["group"]                                        # a wave's row
    c["wave"] = 64 * c["kCutPer"]                                     # a wave's share of a block
    c["block"] = c["kCutBlock"] * c["kCutPer"]                        # records per block of the walk
    c["chain_block"], c["chain_window"] = c["kCkBlock"], c["kCkBlock"] * c["kCkGrid"]
    c["par_min"] = 16384                                              # account_par_min_records for small tables: one chain window
    assert c["par_min"] == c["chain_window"]
    return c


class Call:
    """recs: the account call. flow: the flow number of every record. cuts: where the evictions on full must happen (indices into
    recs). live_recs: what a first nfagg_ingest folds (None: the table starts empty); live0 flows, numbered 0 .. live0 - 1.
    info: what the builder designed beyond the cuts (segments, fields)."""

    def __init__(self, recs, flow, cuts, max_entries, keys, live_recs=None, live0=0, info=None, deliver=None):
        self.recs, self.flow, self.cuts, self.max_entries, self.keys = recs, flow, list(cuts), max_entries, keys
        self.live_recs, self.live0, self.info = live_recs, live0, info or {}
        self.deliver = deliver                                        # (out_cap, max_epochs) of every nfagg_account, or None: the defaults

    def everything(self):
        """The first call's records and the account call's, as the oracle's Accounter sees them."""
        return self.recs if self.live_recs is None else np.concatenate([self.live_recs, self.recs])


def key_pool(O, count, seed):
    """count distinct 40-byte keys (byte 39 zero) of a variant-1 stream, in an order that has nothing to do with their bytes."""
    src = O.gen_stream(2 * count + 4096, seed=1000 + seed, n_keys=1 << 26, variant=1)
    raw = np.ascontiguousarray(src.view(np.uint8).reshape(-1, 144)[:, :40])
    raw[:, 39] = 0
    uniq = np.unique(raw.view(np.dtype((np.void, 40))).reshape(-1)).view(np.uint8).reshape(-1, 40)
    assert len(uniq) >= count, (len(uniq), count)
    return np.ascontiguousarray(uniq[np.random.default_rng(seed).permutation(len(uniq))[:count]])


def materialize(O, flow, keys, seed):
    """One record per entry of flow: a variant-1 base (every order-dependent field of AccumulateBase scrambled, zeros included)
    with keys[flow[i]] written over key bytes 0..38 of record i; byte 39 stays as the base dirtied it."""
    flow = np.asarray(flow, dtype=np.int64)
    base = O.gen_stream(len(flow), seed=seed, n_keys=1 << 16, variant=1)
    raw = base.view(np.uint8).reshape(len(flow), 144)
    raw[:, :39] = keys[flow, :39]
    return base


# ---------------------------------------------------------------- cuts where the plan says
def plan_flows(n, max_entries, cuts, rng, live0=0, heads=None, first_live=0, tail_heads=None):
    """The flow number of every record of a call of n records that is cut exactly at `cuts` (strictly increasing; cuts[0] may be
    0 when live0 == max_entries). Flows 0 .. live0 - 1 are live in the table when the call starts; fresh flows are numbered
    from live0 on IN ORDER OF APPEARANCE. heads = {epoch: positions of its first occurrences} overrides the random placement
    (epoch t = [bounds[t], bounds[t + 1]) with bounds = [0, *cuts, n]; the positions include the epoch's first record where
    that is a head). first_live: the first records of the call repeat live flows. Returns (flow, n_flows, reused) — reused: how
    many heads are flows with an earlier record in the call."""
    M, cuts = max_entries, [int(c) for c in cuts]
    bounds = [0, *cuts, n]
    assert all(b > a for a, b in zip(cuts, cuts[1:])) and (not cuts or (0 <= cuts[0] and cuts[-1] < n))
    assert 0 <= live0 <= M and first_live <= (bounds[1] if live0 else 0)
    flow = np.full(n, -1, dtype=np.int64)
    fresh = live0
    sets = []                                                         # the flows of every epoch so far
    reused = heads_later = 0
    for t in range(len(bounds) - 1):
        a, b = bounds[t], bounds[t + 1]
        last = t == len(bounds) - 2
        seen = list(range(live0)) if t == 0 else []
        in_epoch = set(seen)
        if t == 0:
            want = M - live0 if cuts else min(M - live0, tail_heads if tail_heads is not None else M - live0)
        elif last:
            want = min(M, b - a, tail_heads if tail_heads is not None else max(1, M // 2))
        else:
            want = M
        opens = t > 0 or live0 == 0                                   # the epoch's first record is a head
        if heads and t in heads:
            hp = sorted(int(x) for x in heads[t])
        else:
            lo = a + (1 if opens else max(first_live, 1))
            k = want - (1 if opens and want else 0)
            assert k == 0 or b - lo >= k, "epoch %d: %d records for %d more heads" % (t, b - lo, k)
            hp = sorted(([a] if opens and want else []) + ((lo + rng.choice(b - lo, size=k, replace=False)).tolist() if k else []))
        assert len(hp) == want and len(set(hp)) == want and all(a <= p < b for p in hp), (t, want, len(hp))
        assert not (opens and want) or hp[0] == a
        assert want or a == b or not opens, "an epoch of a full table that has records must start the call"
        is_head = np.zeros(b - a, dtype=bool)
        is_head[np.asarray(hp, dtype=np.int64) - a] = True
        before = list(sets[-1]) if sets else []                       # the epoch directly before: its flows are new here
        older = [f for f in sets[-2] if f not in sets[-1]] if len(sets) >= 2 else []
        rng.shuffle(before); rng.shuffle(older)

        def take(pool):
            while pool:
                f = pool.pop()
                if f not in in_epoch:
                    return f
            return None

        for i in range(a, b):
            if is_head[i - a]:
                f = None
                u = rng.random()
                if t > 0:
                    heads_later += 1
                    if 5 * reused < 2 * heads_later:                  # never by chance below a third of the heads
                        u = 0.0
                if i == a and t > 0:                                  # it found the map full: not a flow of the ending epoch
                    if u < 0.5:
                        f = take(older)
                elif u < 0.5:
                    f = take(before)
                    if f is None:
                        f = take(older)
                elif u < 0.7:
                    f = take(older)
                if f is None:
                    f = fresh; fresh += 1
                else:
                    reused += 1
                seen.append(f); in_epoch.add(f)
            else:
                assert seen, "record %d repeats a flow, and the epoch has none yet" % i
                f = seen[int(rng.integers(len(seen)))]
            flow[i] = f
        sets.append(in_epoch)
    assert (flow >= 0).all()
    return flow, fresh, reused


def cut_call(O, n, max_entries, cuts, seed, live=0, heads=None, first_live=0, tail_heads=None, special=None, deliver=None, live_repeat=2):
    """A call of n records that the evict-on-full loop cuts exactly at `cuts`. live: flows a first nfagg_ingest leaves in the table
    (Call.live_recs: every live flow live_repeat times, shuffled). special = {flow number: 40-byte key} replaces pool keys (the
    fresh flows are numbered from `live` on in order of appearance: with an empty table the first epoch's heads are all fresh)."""
    rng = np.random.default_rng(seed)
    flow, n_flows, reused = plan_flows(n, max_entries, cuts, rng, live, heads, first_live, tail_heads)
    keys = key_pool(O, n_flows, seed)
    for f, k in (special or {}).items():
        assert f < n_flows
        keys[f] = k
    assert len(np.unique(keys.view(np.dtype((np.void, 40))).reshape(-1))) == n_flows
    recs = materialize(O, flow, keys, 2 * seed + 1)
    live_recs = None
    if live:
        lf = np.repeat(np.arange(live), live_repeat)
        live_recs = materialize(O, lf[rng.permutation(len(lf))], keys, 2 * seed + 2)
    return Call(recs, flow, cuts, max_entries, keys, live_recs, live, {"reused_heads": reused}, deliver=deliver)


def spaced(points, gap):
    """The points dealt into as few increasing lists as a greedy pass needs so that neighbours in a list are >= gap apart."""
    lists = []
    for p in sorted(set(points)):
        for l in lists:
            if p - l[-1] >= gap:
                l.append(p)
                break
        else:
            lists.append([p])
    return lists


# ---------------------------------------------------------------- segments of a chosen length
def _interleave(L, c, at):
    """'h' x L and 'c' x c in one order: `at` records of the hot flow, then the collider's first, the rest spread evenly."""
    if not c:
        return ["h"] * L
    assert 1 <= at <= L
    rest = [(i / c, "c") for i in range(c)] + [((j + 0.5) / (L - at), "h") for j in range(L - at)]
    return ["h"] * at + [x for _, x in sorted(rest)]


def segment_call(O, max_entries, lengths, colliders, seed, n_min=None):
    """A lead epoch, one MIDDLE epoch per entry of lengths, a tail (only complete middle epochs are segment-folded). In middle epoch
    k one flow (the hot flow) has exactly lengths[k] records; colliders[k] = None or (c, at): a second flow with the same 64-bit
    key hash has c records, the first of them after `at` records of the hot flow, the others spread evenly among the rest of the
    hot flow's: the hot flow's segment then counts lengths[k] + c sorted positions and folds lengths[k] records. The epoch is
    filled to max_entries flows with flows of one record each, at random places (some of them, never the epoch's first record,
    are single-record flows of the epoch before: previous occurrence >= 0, still new). The lead's max_entries flows are
    repeated until the call has n_min records.
    info["segments"][k] = dict(epoch: the eviction's number, L, c, at, hot, col: flow numbers (col -1: none), lo, hi: the epoch)."""
    M = max_entries
    rng = np.random.default_rng(seed)
    colliders = list(colliders) if colliders is not None else [None] * len(lengths)
    assert len(colliders) == len(lengths) and M >= 3
    n_min = constants()["par_min"] if n_min is None else n_min
    fresh = [0]

    def new_flow():
        fresh[0] += 1
        return fresh[0] - 1

    pairs, middle, segs, prev_singles = [], [], [], []
    for k, L in enumerate(lengths):
        c, at = colliders[k] if colliders[k] else (0, 0)
        hot = new_flow()
        col = new_flow() if c else -1
        if c:
            pairs.append((hot, col))
        body = [hot if x == "h" else col for x in _interleave(L, c, at)]
        n_single = M - 1 - (1 if c else 0)
        pool = list(prev_singles)
        rng.shuffle(pool)
        singles = [pool.pop() if (s > 0 and pool and rng.random() < 0.5) else new_flow() for s in range(n_single)]
        # the epoch's first record is a fresh single (k even) or the hot flow's first (k odd): never a flow of the epoch before
        if k % 2 == 0:
            order, rest = [singles[0]], singles[1:]
        else:
            order, rest = [body.pop(0)], singles
        slots = sorted(rng.integers(0, len(body) + 1, size=len(rest)).tolist())
        si = 0
        for pos in range(len(body) + 1):
            while si < len(rest) and slots[si] == pos:
                order.append(rest[si]); si += 1
            if pos < len(body):
                order.append(body[pos])
        assert len(order) == L + c + n_single
        middle.append(order)
        segs.append({"epoch": k + 1, "L": L, "c": c, "at": at, "hot": hot, "col": col})
        prev_singles = singles
    tail = [new_flow() for _ in range(min(M, 3))]
    tail = tail + tail[:2]
    lead_flows = [new_flow() for _ in range(M)]
    lead_len = max(M, n_min - sum(len(m) for m in middle) - len(tail))
    lead = lead_flows + [lead_flows[int(x)] for x in rng.integers(0, M, size=lead_len - M)]
    flow = np.array(lead + [f for m in middle for f in m] + tail, dtype=np.int64)
    cuts, at_rec = [], len(lead)
    for k, m in enumerate(middle):
        cuts.append(at_rec)
        segs[k]["lo"], segs[k]["hi"] = at_rec, at_rec + len(m)
        at_rec += len(m)
    cuts.append(at_rec)                                               # the tail's first record ends the last middle epoch
    keys = key_pool(O, fresh[0], seed)
    if pairs:
        crafted = kc.craft(np.repeat(kc._distinct(rng, len(pairs)), 2), rng)
        for j, (h, cl) in enumerate(pairs):
            keys[h], keys[cl] = crafted[2 * j], crafted[2 * j + 1]
    recs = materialize(O, flow, keys, 2 * seed + 1)
    return Call(recs, flow, cuts, M, keys, info={"segments": segs})


# ---------------------------------------------------------------- the record of a segment that decides a field
def rule_fold(r):
    """What AccumulateBase (pkg/model/flow_content.go:28-61) leaves in the order-dependent fields after the records r of ONE flow
    in arrival order, by each field's rule: start the smallest non-zero, end the largest, eth_protocol / dscp / sampling the last
    non-zero, the MACs the first non-zero."""
    m = r["metrics"]

    def last_nz(v):
        nz = np.nonzero(v)[0]
        return int(v[nz[-1]]) if len(nz) else 0

    def first_mac(v):
        nz = np.nonzero(v.any(axis=1))[0]
        return bytes(v[nz[0]]) if len(nz) else bytes(6)

    st = m["start"][m["start"] != 0]
    return {"start": int(st.min()) if len(st) else 0, "end": int(m["end"].max()), "eth_protocol": last_nz(m["eth_protocol"]),
            "dscp": last_nz(m["dscp"]), "sampling": last_nz(m["sampling"]), "src_mac": first_mac(m["src_mac"]), "dst_mac": first_mac(m["dst_mac"])}


def fields_of(rec):
    m = rec["metrics"]
    return {"start": int(m["start"]), "end": int(m["end"]), "eth_protocol": int(m["eth_protocol"]), "dscp": int(m["dscp"]),
            "sampling": int(m["sampling"]), "src_mac": bytes(m["src_mac"]), "dst_mac": bytes(m["dst_mac"])}


END_HI, END_LO = (5 << 32) | 1, (4 << 32) | 0xFFFFFFFF                # the larger one has the smaller low half


def field_call(O, max_entries, specs, seed):
    """A segment_call (one middle epoch per spec, no colliders) whose hot flows carry designed order-dependent fields. spec =
    dict(L, kind, nz):
      "nz"          every order-dependent field zero on all L records but those numbered nz (one or two, in arrival order from 0),
                    which carry non-zero values, different ones per record — for two records the EARLIER one holds the larger
                    eth_protocol, dscp, sampling and end and the smaller MAC bytes, so "the last" and "the largest" differ
      "start_only"  start zero on every record but nz[0]; the other fields as the stream scrambled them
      "end_high"    nz = [k1, k2]: end = END_HI at k1 and END_LO at k2 (the high half decides), the stream's small values elsewhere
      "head_zero"   the first record all-zero in these fields (start included), the others as the stream scrambled them
    Every segment gets "idx" (its records in the call), "expect" (field -> value, from the DESIGNED record: last or first as the
    field's rule says) and "kind"."""
    call = segment_call(O, max_entries, [s["L"] for s in specs], None, seed)
    m = call.recs["metrics"]
    for spec, seg in zip(specs, call.info["segments"]):
        idx = np.nonzero(call.flow == seg["hot"])[0]
        assert len(idx) == spec["L"] and seg["lo"] <= idx[0] and idx[-1] < seg["hi"]
        kind, nz = spec["kind"], list(spec.get("nz", []))
        seg["kind"], seg["nz"], seg["idx"] = kind, nz, idx
        if kind == "nz":
            for f in ORDER_FIELDS:
                m[f][idx] = 0
            assert 1 <= len(nz) <= 2 and nz == sorted(set(nz))
            for j, k in enumerate(nz):
                i = idx[k]
                m["eth_protocol"][i] = (0x86DD, 0x0800)[j]; m["dscp"][i] = (46, 7)[j]; m["sampling"][i] = (0x80000001, 50)[j]
                m["src_mac"][i] = (2, 0, 0, 0, j, 1 + j); m["dst_mac"][i] = (2, 0, 0, 9, j, 7 + j)
                m["start"][i] = (5000, 4000)[j]; m["end"][i] = ((9 << 32) | 5, (8 << 32) | 0xFFFFFFF0)[j]
            first, last = call.recs[idx[nz[0]]], call.recs[idx[nz[-1]]]
            seg["expect"] = {**{f: fields_of(last)[f] for f in ("eth_protocol", "dscp", "sampling", "start")},
                             **{f: fields_of(first)[f] for f in ("src_mac", "dst_mac", "end")}}
        elif kind == "start_only":
            m["start"][idx] = 0
            m["start"][idx[nz[0]]] = 123456
            seg["expect"] = {"start": 123456}
        elif kind == "end_high":
            assert int(m["end"][idx].max()) < 1 << 32
            m["end"][idx[nz[0]]], m["end"][idx[nz[1]]] = END_HI, END_LO
            seg["expect"] = {"end": max(END_HI, END_LO)}
        elif kind == "head_zero":
            for f in ORDER_FIELDS:
                m[f][idx[0]] = 0
            seg["expect"] = rule_fold(call.recs[idx[1:]]) if len(idx) > 1 else {f: fields_of(call.recs[idx[0]])[f] for f in ORDER_FIELDS}
        else:
            raise KeyError(kind)
        if kind == "end_high" and spec.get("swap"):
            m["end"][idx[nz[0]]], m["end"][idx[nz[1]]] = END_LO, END_HI
    return call


def field_specs(L, consts):
    """The specs of one segment length: the single non-zero record at every k of the list that fits, the two-record variant for
    every adjacent pair, start on one record only, the 64-bit end both ways round, the all-zero head."""
    H, C = consts["H"], consts["C"]
    ks = sorted({k for k in (0, 1, 63, 64, 65, 255, 256, C - 1, C, H - 1, H, L - 1) if 0 <= k < L})
    specs = [{"L": L, "kind": "nz", "nz": [k]} for k in ks]
    specs += [{"L": L, "kind": "nz", "nz": [a, b]} for a, b in zip(ks, ks[1:])]
    specs += [{"L": L, "kind": "start_only", "nz": [ks[len(ks) // 2]]}, {"L": L, "kind": "end_high", "nz": [ks[0], ks[-1]]},
              {"L": L, "kind": "end_high", "nz": [ks[1], ks[-2]] if len(ks) > 3 else [ks[0], ks[-1]], "swap": True}, {"L": L, "kind": "head_zero"}]
    return specs


# ---------------------------------------------------------------- the calls both test files use
ONE_HOME_K = 64
ONE_HOME_LOW = (1 << 21) - 1                                          # home slot = the LAST slot of every table of up to 2^21 slots
EDGE_HASHES = (0, 1, 2, M64)                                          # the free marker, its neighbour, the busy marker, all ones
LIVE_M, LIVE0 = 300, 100
BIG_M = 250                                                           # "about 300", and the first epoch can still end at record 255


def _seed(name):
    return zlib.crc32(name.encode()) & 0xFFFFF


def cases(consts=None):
    """name -> builder(O) of every call of the crafted-epoch tests."""
    c = consts or constants()
    G, R, W, B, S, H, C = c["group"], c["row"], c["wave"], c["block"], c["S"], c["H"], c["C"]
    out = {}
    n_pos = 4 * B + 4464
    quad = [40000, 40001, 40002, 40003]                               # one group of four: four consecutive cuts (max_entries 1)
    assert quad[0] % G == 0
    edges = [R - 1, R, R + 1, W - 1, W, W + 1, B - 1, B, B + 1, 4 * B - 1, 4 * B]
    for M in (1, 2, 5, BIG_M):
        pts = edges + (quad if M == 1 else [quad[2]])                 # record index = 0, 1, 2, 3 mod 4 among them
        assert {p % G for p in pts} == set(range(G))
        for j, cuts in enumerate(spaced(pts, M)):
            name = "cuts_m%d_%d" % (M, j)
            out[name] = (lambda O, M=M, cuts=cuts, name=name: cut_call(O, n_pos, M, cuts, _seed(name)))
    # an epoch that begins in a block's last group of four and ends in the next block's first
    out["cuts_straddle"] = lambda O: cut_call(O, 24000, 2, [100, B - 2, B + 1, 20000], _seed("cuts_straddle"))
    # no new flow for two whole blocks: `before` is carried, the counting finds nothing
    out["cuts_quiet_blocks"] = lambda O: cut_call(O, 3 * B + 11000, 5, [201, 402, 703, 1001, 3 * B + 2849, 3 * B + 5002], _seed("cuts_quiet_blocks"),
                                                 heads={4: [1001, 1002, 1003, 1004, 1005]})
    out["cuts_last_record"] = lambda O: cut_call(O, 20000, 5, [3001, 9002, 19999], _seed("cuts_last_record"))
    out["cuts_exact_block"] = lambda O: cut_call(O, B, 5, [501, 8002, B - 1], _seed("cuts_exact_block"))
    out["cuts_block_plus_1"] = lambda O: cut_call(O, B + 1, 5, [503, 8001, B], _seed("cuts_block_plus_1"))
    out["cuts_four_blocks"] = lambda O: cut_call(O, 4 * B, BIG_M, [3001, 30002, 4 * B - 1], _seed("cuts_four_blocks"))
    # room for two evictions per call: the walk stops at max_cuts, NFAGG_TRUNCATED, the next call starts at a cut
    out["cuts_truncated"] = lambda O: cut_call(O, n_pos, BIG_M, [3001, 9002, 15003, 21000, 27001, 33002], _seed("cuts_truncated"), deliver=(2 * BIG_M + 10, 64))
    # ---- a live table
    out["live_full_new"] = lambda O: cut_call(O, 20000, LIVE_M, [0, 6000, 13000], _seed("live_full_new"), live=LIVE_M)
    out["live_full_after_7"] = lambda O: cut_call(O, 20000, LIVE_M, [7, 6000, 13000], _seed("live_full_after_7"), live=LIVE_M, first_live=7)
    out["live_part"] = lambda O: cut_call(O, 20000, LIVE_M, [5000, 11000, 17000], _seed("live_part"), live=LIVE0, first_live=3)

    def special_call(name, targets_live, targets_new):
        def build(O):
            rng = np.random.default_rng(_seed(name) + 1)
            keys = kc.craft(np.concatenate([targets_live, targets_new]), rng)
            sp = {f: keys[f] for f in range(len(targets_live))}
            sp.update({LIVE0 + j: keys[len(targets_live) + j] for j in range(len(targets_new))})
            call = cut_call(O, 20000, LIVE_M, [5000, 11000, 17000], _seed(name), live=LIVE0, special=sp)
            call.info["special"] = sorted(sp)
            return call
        return build

    fam = (kc._distinct(np.random.default_rng(5), ONE_HOME_K, 43) << np.uint64(21)) | np.uint64(ONE_HOME_LOW)
    out["live_one_home"] = special_call("live_one_home", fam[:ONE_HOME_K // 2], fam[ONE_HOME_K // 2:])
    e = np.array(EDGE_HASHES, dtype=np.uint64)
    out["live_edges"] = special_call("live_edges", e, e)
    h = kc._distinct(np.random.default_rng(6), 1)
    out["live_same64"] = special_call("live_same64", h, h)
    # ---- segment lengths
    lengths = [1, 2, S - 1, S, S + 1, S + 2, 63, 64, 65, 255, 256, 257, H - 1, H, H + 1, H + 2, H + C, H + C + 1, 2 * H + 1]
    out["seg_lengths"] = lambda O: segment_call(O, 6, lengths, None, _seed("seg_lengths"))
    # ... reached by POSITIONS: L + c crosses S (H), L alone does not; and the collider the longer one
    pos = [(S - 6, (8, 1)), (S, (1, S)), (S - 1, (1, 1)), (H - 6, (10, 1)), (H, (1, 7)), (5, (2 * S, 1)), (S + 4, (H - 10, 2))]
    out["seg_positions"] = lambda O: segment_call(O, 5, [l for l, _ in pos], [cl for _, cl in pos], _seed("seg_positions"))
    # ... a collider's head inside the hot flow's run: both long, both huge, a short one inside a long one
    ins = [(100, (60, 30)), (H + 900, (H + 400, 200)), (40, (3, 30)), (S + 4, (S + 4, S // 2))]
    out["seg_inside"] = lambda O: segment_call(O, 7, [l for l, _ in ins], [cl for _, cl in ins], _seed("seg_inside"))
    sk = [(1, None), (S + 1, None), (300, (20, 5)), (H + 1, None), (H + C + 1, None)]

    def sketch_call(O):
        call = segment_call(O, 4, [l for l, _ in sk], [cl for _, cl in sk], _seed("seg_sketch"))
        call.info["sketch"] = True
        return call

    out["seg_sketch"] = sketch_call
    # ---- which record of a segment decides a field: a short, a long and a huge segment
    out["field_short"] = lambda O: field_call(O, 4, field_specs(12, c), _seed("field_short"))
    out["field_long"] = lambda O: field_call(O, 4, field_specs(700, c), _seed("field_long"))
    huge = field_specs(H + C + 300, c)
    per = 9
    for j in range(0, len(huge), per):
        name = "field_huge_%d" % (j // per)
        out[name] = (lambda O, j=j, name=name: field_call(O, 4, huge[j:j + per], _seed(name)))
    return out


_CACHE = {}


def get(O, name):
    """The call of one case, built once per process."""
    if name not in _CACHE:
        _CACHE[name] = cases()[name](O)
    return _CACHE[name]


# ---------------------------------------------------------------- what the kernels will see, from the numpy model's sort keys
IDX_BITS = 24
IDX = (1 << IDX_BITS) - 1


def segment_positions(ks, i, epoch_end):
    """Sorted positions of the segment whose head is record i: from its own position up to the first key that reaches (its hash
    bits, epoch_end) — what k_par_segfold compares with kSegShort and kSegHuge."""
    inv = np.empty(len(ks), dtype=np.int64)
    inv[(ks & np.uint64(IDX)).astype(np.int64)] = np.arange(len(ks))
    p = int(inv[i])
    limit = (int(ks[p]) & ~IDX) | int(epoch_end)
    return int(np.searchsorted(ks, np.uint64(limit), side="left")) - p


def seg_class(positions, consts):
    return "short" if positions <= consts["S"] else ("long" if positions <= consts["H"] else "huge")
