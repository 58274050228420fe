"""k_pb_write's window loop beyond its first iteration (csrc/nfagg_pb.hip), all three instantiations, Accounter and content
encoding, host and device entry points: streams in which runs of the longest frames stand among short ones (tests/
pb_window_mixes.py), so that waves span two to four LDS windows and frames lie across the borders — behind a frame's 0x0A,
inside its length varint, before and behind its last byte — under every value of wave_base & 15. Each stream's preconditions
are asserted from the oracle's frame lengths before the product's bytes are compared with the oracle's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pb_window_mixes as M  # noqa: E402
from test_pb_gpu import AGENT4, NAMES, _records_of, _split_contents, frames  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tab(nf):
    with nf.FlowTable(max_entries=64) as t:
        yield t


def device_encode(nf, tab, recs, present, parts):
    """Size query, then the write, through nfagg_encode_pb[_content]_device; 64 guard bytes behind `need` stay 0xAB."""
    import torch
    n = len(recs)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_recs = dev(recs)
    kw = {}
    if present is not None:
        d_present, d_parts = dev(present), {k: dev(v) for k, v in parts.items()}
        kw = dict(d_present=d_present.data_ptr(), d_parts={k: v.data_ptr() for k, v in d_parts.items()})
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_len = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_keys = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    args = (d_recs.data_ptr(), n, M.NOW, M.MONO, AGENT4, nf.intf_table(NAMES))
    rc, need = tab.encode_pb_device(*args, 0, 0, d_off.data_ptr(), d_len.data_ptr(), **kw)
    assert rc == nf.TRUNCATED and need > 0
    d_out = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    rc, wrote = tab.encode_pb_device(*args, d_out.data_ptr(), need, d_off.data_ptr(), d_len.data_ptr(), d_keys.data_ptr(), **kw)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert rc == nf.OK and wrote == need and (out[need:] == 0xAB).all()
    return out[:need], d_off.cpu().numpy().astype(np.uint64), d_len.cpu().numpy().astype(np.uint32), d_keys.cpu().numpy().reshape(n, 32)


def check(got, want, want_keys, label):
    buf, off, blen, keys = got
    assert int(off[0]) == 0 and int(off[-1]) == len(buf) and (np.diff(off.astype(np.int64)) > 0).all(), label
    assert blen.tolist() == [len(b) for b in want], label
    got_bodies = frames(buf, off, blen)
    if got_bodies != want:
        k = next(i for i, (a, b) in enumerate(zip(got_bodies, want)) if a != b)
        j = next(i for i, (a, b) in enumerate(zip(got_bodies[k], want[k])) if a != b)
        raise AssertionError("%s: frame %d differs from byte %d of its body on: got %s want %s"
                             % (label, k, j, got_bodies[k][j:j + 8].hex(), want[k][j:j + 8].hex()))
    assert np.array_equal(keys, want_keys), label


@pytest.mark.parametrize("content", [False, True], ids=["accounter", "content"])
@pytest.mark.parametrize("window", sorted(M.MIXES))
def test_frames_across_windows_match_the_oracle(nf, O, tab, window, content):
    variants = M.sweep(O, NAMES, AGENT4, window, content)
    M.check_preconditions(window, variants)
    want_keys = O.kafka_keys(variants[0][1])                      # the addresses are the same in every variant
    for label, recs, contents, want in variants:
        present = parts = None
        product_recs = recs.view(nf.FLOW_RECORD)
        if content:
            present, parts = _split_contents(nf, O, contents)
            product_recs = _records_of(nf, O, recs["id"], contents)
        got = tab.encode_pb(product_recs, M.NOW, M.MONO, AGENT4, nf.intf_table(NAMES), kafka_keys=True, present=present, parts=parts)
        check(got, want, want_keys, label + " (host)")
        check(device_encode(nf, tab, product_recs, present, parts), want, want_keys, label + " (device)")
