"""The value edges of tests/test_flp_json_gpu.stream through the protobuf and IPFIX encoders (csrc/nfagg_pb.hip, nfagg_ipfix.hip):
times ahead of the clock by a wrap and start = 2^63 + ..., Bytes = 2^64 - 1 (a ten-byte varint), Packets = 2^32 - 1, sparse v6
groups, a non-IP ethertype — under a clock before 1970, where put_time's seconds are negative (ten bytes, which the size kernel
must count too) and IPFIX sends uint32(t.Unix()) and uint64(t.UnixMilli()) of a negative time. Expected bytes: the C oracle
(pinned on these edges against the protobuf runtime by tests/test_pb_oracle.py) and tests/ipfix_ref.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ipfix_ref as IR  # noqa: E402
import test_flp_json_gpu as G  # noqa: E402
from test_flp_json_content_gpu import content_parts  # noqa: E402
from test_pb_gpu import AGENT4, NAMES, _records_of, _split_contents, frames  # noqa: E402

pytestmark = pytest.mark.gpu

NOW, MONO = G.NOW, G.MONO                       # MONO = 2.5 ms: end = 2^64 - 5 is ahead of the clock
AGENT6 = bytes.fromhex("fd00000000000000000000000000000a")
EXPORT = 1_700_000_000


def clocks_and_agents():
    """The four (now, agent) pairs: today's clock, 5 ns after the epoch, 11.6 days and 3.2 years before it."""
    return [(NOW, AGENT4), (5, bytes(np.random.default_rng(16).integers(0, 256, 16, dtype=np.uint8))), (-10**15, AGENT6), (-10**17, AGENT4)]


def flow_time(now, mono, ts):
    """record.go:90-97 in Python integers: now.Add(-Duration(mono - ts)), the subtraction and the negation wrapping in int64."""
    delta = (mono - ts) % 2**64
    d = -(delta - 2**64 if delta >= 2**63 else delta)
    return now + (d if d < 2**63 else d - 2**64)


def oracle_contents(nf, O, recs, present, parts):
    """(present, parts) of content_parts -> the oracle's CONTENT array over these records (network events: the bit alone)."""
    n = len(recs)
    c = np.zeros(n, dtype=O.CONTENT)
    c["base"] = recs.view(O.FLOW_RECORD)["metrics"]
    for kind, has, bit in (("additional", "has_additional", nf.FEAT_ADDITIONAL), ("dns", "has_dns", nf.FEAT_DNS), ("drops", "has_drops", nf.FEAT_DROPS),
                           ("xlat", "has_xlat", nf.FEAT_XLAT), ("quic", "has_quic", nf.FEAT_QUIC)):
        c[kind] = np.ascontiguousarray(parts[kind]).view(np.uint8).reshape(n, -1).copy().view(O.KIND_DTYPES[O.KIND_INDEX[kind]]).reshape(n)
        c[has] = (present & bit) != 0
    c["has_netev"] = (present & nf.FEAT_NETWORK_EVENTS) != 0
    return c


def assert_stream_has_the_edges(recs):
    m = recs["metrics"]
    assert (m["end_mono_time_ts"] == 2**64 - 5).any() and (m["start_mono_time_ts"] == 2**63 + 12345).any() and (m["start_mono_time_ts"] == 0).any()
    assert (m["bytes"] == 2**64 - 1).any() and (m["packets"] == 2**32 - 1).any()
    assert (m["eth_protocol"] == 0x0806).any() and (m["eth_protocol"] == 0x86DD).any()


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


@pytest.mark.parametrize("n", [65, 1025, 5000])
def test_protobuf_edge_values_match_the_oracle(nf, O, tab, n):
    recs = G.stream(nf, O, n, seed=n + 11, keep_tls=True)
    assert_stream_has_the_edges(recs)
    present, parts = content_parts(nf, n, seed=n + 12)
    contents = oracle_contents(nf, O, recs, present, parts)
    p_present, p_parts = _split_contents(nf, O, contents)
    assert np.array_equal(p_present, present)
    orecs = recs.view(O.FLOW_RECORD)
    want_keys = O.kafka_keys(orecs)
    for now, agent in clocks_and_agents():
        opts = O.pb_options(now, MONO, agent, O.intf_table(NAMES))
        want = O.pb_encode(orecs, opts)
        if now < 0:                                                   # negative seconds (ten bytes) on most records; start = 2^63 + ... is far ahead
            neg = [flow_time(now, MONO, int(t)) < 0 for t in recs["metrics"]["start_mono_time_ts"]]
            assert 0.5 * n < sum(neg) < n
        buf, off, blen, keys = tab.encode_pb(recs, now, MONO, agent, nf.intf_table(NAMES), kafka_keys=True)
        assert frames(buf, off, blen) == want, now
        assert int(off[0]) == 0 and int(off[-1]) == len(buf) and (np.diff(off.astype(np.int64)) > 0).all()
        assert np.array_equal(keys, want_keys)
        want_c = O.pb_encode_contents(orecs["id"], contents, opts)
        buf, off, blen = tab.encode_pb(_records_of(nf, O, orecs["id"], contents), now, MONO, agent, nf.intf_table(NAMES), present=p_present, parts=p_parts)
        assert frames(buf, off, blen) == want_c, now
        assert int(off[0]) == 0 and int(off[-1]) == len(buf) and (np.diff(off.astype(np.int64)) > 0).all()


@pytest.mark.parametrize("n", [65, 1025, 5000])
def test_ipfix_edge_values_match_the_restatement(nf, O, tab, n):
    recs = G.stream(nf, O, n, seed=n + 11, keep_tls=True)
    assert_stream_has_the_edges(recs)
    rows = [(i, m, name.encode()) for (i, m, name, _) in NAMES]
    for now, _ in clocks_and_agents():
        want, want_off = IR.encode(recs, now, MONO, rows, EXPORT, 0xFFFFFF00 + n)
        buf, off = tab.encode_ipfix(recs, now, MONO, nf.intf_table(NAMES), EXPORT, 0xFFFFFF00 + n)
        assert off.tolist() == want_off.tolist(), now
        assert buf.tobytes() == want, now
