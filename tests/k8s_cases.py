"""Inputs the Kubernetes tests share (tests/test_flp_json_k8s_cpu.py, test_flp_json_k8s_gpu.py): an informer answer whose
block has an exact size, and the flow whose enriched line is the longest each policy can write."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_k8s_ref as K  # noqa: E402
import tls_worst_case as W  # noqa: E402

KEY_TEXT = 181          # ,"SrcK8S_<key>":"" over the nine keys


def info_of_block_size(total: int, escaped: bool = False) -> dict:
    """Every key present, the block exactly `total` bytes on either side. escaped: the name is bytes that escape six-fold
    (as many as fit, the rest plain), so that the host escapes into the cap's last byte."""
    info = dict(namespace="x", kind="k", owner_name="o", owner_kind="t", network_name="p", host_ip="h", host_name="m", zone="z")
    room = total - KEY_TEXT - 8
    assert room >= 0
    info["name"] = b"\x01" * (room // 6) + b"n" * (room % 6) if escaped else b"n" * room
    assert len(K.render("::1", info, 0)) == len(K.render("::1", info, 1)) == total
    return info


INFRA_LAYER = (["x"], [])           # namespace "x" is infrastructure: the longer of the two layer values


def worst_case(nf, n, policy):
    """tls_worst_case.worst_case plus a table row for the flow's address (src == dst) whose two blocks have 2048 bytes."""
    case = W.worst_case(nf, n, policy)
    case["k8s"] = [(W.V6, info_of_block_size(K.MAX_RENDERED, escaped=True))]
    case["layer"] = INFRA_LAYER
    return case


def reference(case):
    """(bytes, offsets) of the restatement for a case of worst_case()."""
    present, parts, events = case["present"], case["parts"], None
    if case["answers"] is not None:
        present, drops, _rows, events, missing = W.RN.resolve(present, parts["network_events"], parts["drops"], case["answers"])
        assert not missing
        parts = {**parts, "drops": drops.view(parts["drops"].dtype).reshape(-1)}
    return K.encode(case["recs"], W.T.table_of(case["tls"]), K.table_of(case["k8s"]), case["layer"], case["now"], case["mono"], case["names"],
                    case["agent"], case["received"], present=present, parts=parts, events=events)
