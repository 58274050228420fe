"""Pins the oracle's kernel-dedup restatement (nfagg_oracle.c: update_existing_flow / add_observed_intf, mode 1) to the
REFERENCE ITSELF: oracle/_ref/libref_flows.so is bpf/flows.c:76-143 + bpf/types.h compiled with host gcc from the
reference checkout (oracle/Makefile target `ref`, oracle/ref_flows_shim.c = the kernel-environment shim).

That library can only be built where the reference checkout is readable, and it is git-ignored. So what it computes on
every stream below is also stored in tests/golden/ref_dedup_golden.json (sha256 of its evictions, written by
tests/golden/gen_ref_dedup_golden.py): a checkout without the library checks the oracle against those digests; a checkout
with it compares the oracle with the reference record for record AND checks that the reference still computes what was stored."""
import hashlib
import json
import os

import numpy as np
import pytest

import dedupcraft
from conftest import assert_records_equal, dedup_stream

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_dedup_golden.json")


def digest(evictions):
    """What a run of evictions is pinned by: their number, their flows, and a sha256 over every reason and record byte."""
    h = hashlib.sha256()
    for reason, recs in evictions:
        h.update(reason.encode() + b"\0" + len(recs).to_bytes(8, "little"))
        h.update(np.ascontiguousarray(recs).tobytes())
    return {"evictions": len(evictions), "flows": int(sum(len(r) for _, r in evictions)), "sha256": h.hexdigest()}


# ---- the streams the reference is run on: name -> (records, max_entries). tests/golden/gen_ref_dedup_golden.py uses the same table.
def flows_c_case(O, style, max_entries):
    th = O.zipf_thresholds(300, 1.1)
    return dedup_stream(O, 40000, seed=200 + style, n_keys=300, thresholds=th, style=style), max_entries


def hot_flow_case(O, seed, style):
    th = O.zipf_thresholds(2000, 1.1)
    return dedup_stream(O, 200000, seed=seed, n_keys=2000, thresholds=th, hot_permille=900, style=style), 1 << 16


def single_packet_case(O):
    recs = dedup_stream(O, 30000, seed=31, n_keys=200, style=2)
    recs["metrics"]["packets"] = 1
    return recs, 1 << 16


def missed_counter_case(O):
    return dedup_stream(O, 20000, seed=202, n_keys=50, style=2), 1 << 16


def direct_case(O):
    """One flow: record 0 is the aggregate, the rest are merged into it one call at a time."""
    recs = dedup_stream(O, 4000, seed=9, n_keys=1, style=2)
    agg = recs[0]["metrics"].copy().reshape(1)
    agg.view(np.uint8).reshape(-1)[66:68] = 0
    agg.view(np.uint8).reshape(-1)[100:104] = 0
    return recs, agg


def script_family_case(name):
    """tests/dedupcraft.py: every order of events over the merge's small alphabets, flow after flow, nothing evicted early."""
    return dedupcraft.family(name).recs, 1 << 20


STYLES, MAX_ENTRIES, HOT = [0, 1, 2, 3], [1 << 20, 50, 1], [(6, 1), (7, 2)]


def stream_cases(O):
    """Every stream whose reference evictions are stored, by name."""
    cases = {}
    for style in STYLES:
        for m in MAX_ENTRIES:
            cases["flows_c[style=%d,max_entries=%d]" % (style, m)] = lambda s=style, m=m: flows_c_case(O, s, m)
    for seed, style in HOT:
        cases["hot_flow[seed=%d,style=%d]" % (seed, style)] = lambda seed=seed, style=style: hot_flow_case(O, seed, style)
    cases["single_packet"] = lambda: single_packet_case(O)
    cases["missed_counter"] = lambda: missed_counter_case(O)
    for name in dedupcraft.FAMILIES:
        cases["scripts[%s]" % name] = lambda name=name: script_family_case(name)
    return cases


def ref_direct(ref, recs, agg):
    """update_existing_flow of the reference on `agg`, once per record after the first."""
    for i in range(1, len(recs)):
        ref.ref_update_existing_flow(agg.ctypes.data, recs[i:i + 1].ctypes.data)
    return agg


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ref(O):
    """The reference's compiled code where this checkout has it, else None (the stored digests stand for it)."""
    return O.ref_lib() if O.ref_available() else None


def same(O, ref, golden, name, recs, max_entries):
    """The oracle's evictions equal the reference's: record for record when the reference is built here, by digest always."""
    got = O.run_accounter(recs, max_entries, mode=1)
    want = golden["streams"][name]
    if ref is not None:
        live = O.run_ref_dedup(recs, max_entries)
        assert [r for r, _ in got] == [r for r, _ in live]
        for k, ((_, g), (_, w)) in enumerate(zip(got, live)):
            assert_records_equal(g, w, f"oracle vs bpf/flows.c, eviction #{k}")
        assert digest(live) == want, f"{name}: the reference no longer computes what tests/golden/ref_dedup_golden.json holds"
    assert digest(got) == want, f"{name}: oracle differs from the stored evictions of bpf/flows.c"
    return got


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("max_entries", MAX_ENTRIES)
def test_oracle_dedup_equals_reference_flows_c(O, ref, golden, style, max_entries):
    recs, _ = flows_c_case(O, style, max_entries)
    got = same(O, ref, golden, "flows_c[style=%d,max_entries=%d]" % (style, max_entries), recs, max_entries)
    if max_entries > 300 and style in (0, 2):   # the streams do reach the capacity cut-off and the BOTH merge
        m = got[0][1]["metrics"]
        assert (m["nb_observed_intf"] == 6).any() and (m["observed_direction"] == 3).any()


def test_oracle_dedup_equals_reference_hot_flow(O, ref, golden):
    """configs[4] shape: 90 % of the records are one flow alternating over interfaces."""
    for seed, style in HOT:
        recs, m = hot_flow_case(O, seed, style)
        same(O, ref, golden, "hot_flow[seed=%d,style=%d]" % (seed, style), recs, m)


def test_single_packet_records_need_no_packet_fixup(O, ref, golden):
    """With packets == 1 per record the shim's `packets - 1` top-up is zero: the reference's arithmetic alone."""
    recs, m = single_packet_case(O)
    same(O, ref, golden, "single_packet", recs, m)


@pytest.mark.parametrize("family", dedupcraft.FAMILIES)
def test_oracle_dedup_equals_reference_on_the_script_families(O, ref, golden, family):
    """The families the device tests of kernel-dedup mode are judged by (tests/test_crafted_dedup_gpu.py): the oracle is the
    reference on every one of their flows."""
    recs, m = script_family_case(family)
    got = same(O, ref, golden, "scripts[%s]" % family, recs, m)
    assert [r for r, _ in got] == ["closing"] and len(got[0][1]) == dedupcraft.family(family).n_scripts


def test_reference_function_directly(O, ref, golden):
    """update_existing_flow on hand-made aggregates, one call at a time, against orc (through a two-record stream)."""
    recs, agg = direct_case(O)
    want = O.run_accounter(recs, 10, mode=1)[0][1]
    stored = golden["direct_metrics_hex"]
    if ref is not None:
        agg = ref_direct(ref, recs, agg)
        assert agg.tobytes() == want["metrics"].tobytes()
        assert agg.tobytes().hex() == stored, "the reference no longer computes what tests/golden/ref_dedup_golden.json holds"
    assert want["metrics"].tobytes().hex() == stored


def test_observed_intf_missed_counter(O, ref, golden):
    """flows.c:133-142: the capacity cut-off is reported (counter raised on non-zero proto)."""
    recs, m = missed_counter_case(O)
    assert golden["missed_counter_observed_intf_missed"] > 0
    if ref is not None:
        ref.ref_counters_reset()
        O.run_ref_dedup(recs, m)
        assert ref.ref_counter_observed_intf_missed() == golden["missed_counter_observed_intf_missed"]
    got = same(O, ref, golden, "missed_counter", recs, m)
    assert any((e["metrics"]["nb_observed_intf"] == 6).any() for _, e in got)     # the oracle's evictions do reach the cut-off
