"""The streams of tests/test_pb_windows_gpu.py, CPU leg: from the oracle's frame lengths alone, every mix takes the window it is
built for (launch_pb_write's rule, read from csrc/nfagg_pb.hip), has waves longer than that window where the runs of long frames
lie, frames across borders, a border inside a frame's `0x0A varint(len)` prefix, one before and one behind a frame's last byte,
and all 16 values of wave_base & 15. So the GPU comparison reaches the second iteration of k_pb_write's window loop in each of
its three instantiations without anybody having to look at the hardware."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pb_window_mixes as M  # noqa: E402
from test_pb_gpu import AGENT4, NAMES  # noqa: E402


def test_window_rule_is_the_one_the_mixes_were_built_for():
    # launch_pb_write (csrc/nfagg_pb.hip): average frame length <= 120 -> 8 KiB, <= 248 -> 16 KiB, else 24 KiB
    assert M.window_rule() == ([120, 248], [8192, 16384, 24576])
    assert sorted(M.MIXES) == M.window_rule()[1]
    assert M.window_for([120] * 3) == 8192 and M.window_for([121, 120, 122]) == 16384      # the average is floored
    assert M.window_for([248]) == 16384 and M.window_for([249]) == 24576


@pytest.mark.parametrize("content", [False, True])
@pytest.mark.parametrize("window", sorted(M.MIXES))
def test_mix_preconditions_hold(O, window, content):
    variants = M.sweep(O, NAMES, AGENT4, window, content)
    assert len(variants) == 20
    M.check_preconditions(window, variants)
    _, recs, contents, bodies = variants[0]
    L = M.frame_lengths(bodies)
    long_ = L > 700
    assert 700 < L[long_].min() and L[long_].max() <= 1033 and L[~long_].max() < 500       # a frame is at most 1033 B
    assert int(long_.sum()) == sum(c for _, c in M.MIXES[window]["runs"])
    if content:
        assert L[long_].min() > 900 and (contents["has_dns"][long_] == 1).all() and not contents["has_dns"][~long_].any()


def test_geometry_on_hand_made_lengths():
    """Two waves of 64 frames, 100 bytes each (body 98), window 4096: wave 0 has its border at image byte 4096 = frame 40, 96
    bytes in; wave 1 starts at byte 6400 (shift 0)."""
    g = M.geometry([100] * 128, [98] * 128, 4096)
    assert g["multi"] == [0, 1] and g["shifts"] == [0, 0] and g["straddle"] == [(40, 96), (104, 96)] and g["largest"] == 6400
    g = M.geometry([4095, 3] + [100] * 62, [4092, 1] + [98] * 62, 4096)                   # border behind frame 1's 0x0A
    assert g["straddle"] == [(1, 1), (42, 94)] and g["in_prefix"] == [1]
    g = M.geometry([4097] + [5] * 63, [4094] + [3] * 63, 4096)
    assert g["last_byte"] == [0] and not g["ends_on"]
    g = M.geometry([7, 4096] + [5] * 62, [5, 4093] + [3] * 62, 4096)                       # wave 0 only; frame 1 ends 7 behind the border
    assert g["straddle"] == [(1, 4089)]
    g = M.geometry([3] * 64 + [4096] + [5] * 63, [1] * 64 + [4093] + [3] * 63, 4096)   # wave 1 starts at 192: shift 0, frame ends on the border
    assert g["ends_on"] == [64] and not g["straddle"]
    g = M.geometry([3] * 63 + [4] + [4095] + [5] * 63, [1] * 63 + [2] + [4092] + [3] * 63, 4096)   # wave 1 starts at 193: shift 1
    assert g["shifts"] == [1] and g["ends_on"] == [64]
