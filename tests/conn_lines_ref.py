"""What extract conntrack's flow logs are expected to be, from the lines of the same records without conntrack: which flows the
stage tracks, and the two keys spliced into a tracked flow's line. No import of the product; shared by tests/test_conn_lines_cpu.py
and tests/test_conn_lines_gpu.py."""
import numpy as np


def tracked(recs):
    """conntrack.go:70-74 with the stage's usual filter: the flows that have SrcPort and DstPort."""
    return np.isin(recs["metrics"]["eth_protocol"], (0x0800, 0x86DD)) & np.isin(recs["id"]["transport_protocol"], (6, 17, 132))


def splice(net_want, recs, ids):
    """(bytes, offsets) of the flow logs from the restatement's (bytes, offsets) of the same records' *_net lines."""
    buf, off = net_want
    keep = tracked(recs)
    lines, offs = [], [0]
    for i in range(len(recs)):
        line = buf[int(off[i]):int(off[i + 1])]
        assert line.endswith(b"}\n")
        lines.append(line[:-2] + b',"_HashId":"%x","_RecordType":"flowLog"}\n' % int(ids[i]) if keep[i] else b"")
        offs.append(offs[-1] + len(lines[-1]))
    return b"".join(lines), np.array(offs, dtype=np.uint64)
