"""Conversations for the tests of the conversation encoder: one spec per conversation, from which come the carrier record and
the nfagg_conn_values row the product takes and, independently, the map tests/conn_json_ref.py marshals."""
import numpy as np

import flp_json_k8s_ref as K
from flp_json_ref import go_ip, go_mac

SNAP_INPUTS = ("TimeFlowStartMs", "TimeFlowEndMs", "SrcAddr", "DstAddr", "SrcPort", "DstPort", "Proto", "SrcMac", "DstMac", "Etype", "Dscp", "IfDirections")
# 32 fields: every operation, split and not, first and last over every input; names that fall around the blocks of the sorted line
FIELDS_32 = ([dict(name="Bytes", operation="sum", splitAB=True), dict(name="Packets", operation="sum", splitAB=True),
              dict(name="numFlowLogs", operation="count", splitAB=True), dict(name="a", operation="count"),
              dict(name="DstB", operation="sum", input="Bytes"), dict(name="_Foo", operation="sum", input="Packets"),
              dict(name="TimeFlowStart", operation="min", input="TimeFlowStartMs"), dict(name="TimeFlowEnd", operation="max", input="TimeFlowEndMs")] +
             [dict(name=n, operation="first", input=i) for n, i in zip(("DstK8", "DstK9", "DstMac", "SrcK8", "SrcSubnetLabe", "K8S_FlowLaye") +
                                                                       tuple("first q\"%d" % k for k in range(6)), SNAP_INPUTS)] +
             [dict(name="last_" + i, operation="last", input=i) for i in SNAP_INPUTS])
FIELDS_COUNT = [dict(name="numFlowLogs", operation="count")]
assert len(FIELDS_32) == 32


def snap(src="10.0.0.1", dst="10.0.0.2", sport=1, dport=2, proto=6, smac=bytes(6), dmac=bytes(6), etype=0x0800, dscp=0, start=0, end=0, dirs=(0,)):
    return dict(src=src, dst=dst, sport=sport, dport=dport, proto=proto, smac=bytes(smac), dmac=bytes(dmac), etype=etype, dscp=dscp, start=start, end=end,
                dirs=tuple(dirs))


def conv(src="10.0.0.1", dst="10.0.0.2", sport=40000, dport=443, proto=6, h=1, rtype="newConnection", is_first=True, flows=(1, 0), nbytes=(100, 0),
         packets=(1, 0), start_min=1000, end_max=2000, first=None, last=None):
    return dict(src=src, dst=dst, sport=sport, dport=dport, proto=proto, h=h, rtype=rtype, is_first=is_first, flows=flows, bytes=nbytes, packets=packets,
                start_min=start_min, end_max=end_max, first=first or snap(src, dst, sport, dport, proto), last=last or snap(dst, src, dport, sport, proto))


def arrays(nf, specs):
    """(carriers FLOW_RECORD[n], values CONN_VALUES[n]) of the specs."""
    n = len(specs)
    car, val = np.zeros(n, dtype=nf.FLOW_RECORD), np.zeros(n, dtype=nf.CONN_VALUES)
    rt = nf._lib.CONN_RECORD_TYPES
    for i, c in enumerate(specs):
        s, d = K.ip16(c["src"]), K.ip16(c["dst"])
        car["id"]["src_ip"][i], car["id"]["dst_ip"][i] = np.frombuffer(s, dtype=np.uint8), np.frombuffer(d, dtype=np.uint8)
        car["id"]["src_port"][i], car["id"]["dst_port"][i], car["id"]["transport_protocol"][i] = c["sport"], c["dport"], c["proto"]
        car["metrics"]["eth_protocol"][i] = 0x86DD if ":" in c["src"] and not c["src"].startswith("::ffff:") else 0x0800
        v = val[i]
        v["hash_total"], v["record_type"], v["is_first"] = c["h"], rt[c["rtype"]], 1 if c["is_first"] else 0
        v["flows"], v["bytes"], v["packets"] = c["flows"], c["bytes"], c["packets"]
        v["start_ms_min"], v["end_ms_max"] = c["start_min"], c["end_max"]
        for which in ("first", "last"):
            q, w = c[which], v[which]
            w["src_ip"], w["dst_ip"] = np.frombuffer(K.ip16(q["src"]), dtype=np.uint8), np.frombuffer(K.ip16(q["dst"]), dtype=np.uint8)
            w["src_port"], w["dst_port"], w["eth_protocol"], w["proto"], w["dscp"] = q["sport"], q["dport"], q["etype"], q["proto"], q["dscp"]
            w["src_mac"], w["dst_mac"] = np.frombuffer(q["smac"], dtype=np.uint8), np.frombuffer(q["dmac"], dtype=np.uint8)
            w["n_dirs"] = len(q["dirs"])
            w["dirs"][:len(q["dirs"])] = q["dirs"]
            w["start_ms"], w["end_ms"] = q["start"], q["end"]
    return car, val


def ref_conv(c):
    """The spec as tests/conn_json_ref.to_map takes it: values as RecordToMap writes them."""
    def values(q):
        return {"SrcAddr": go_ip(K.ip16(q["src"])), "DstAddr": go_ip(K.ip16(q["dst"])), "SrcPort": q["sport"], "DstPort": q["dport"], "Proto": q["proto"],
                "SrcMac": go_mac(q["smac"]), "DstMac": go_mac(q["dmac"]), "Etype": q["etype"], "Dscp": q["dscp"], "TimeFlowStartMs": q["start"],
                "TimeFlowEndMs": q["end"], "IfDirections": list(q["dirs"])}
    keys = {b"SrcAddr": go_ip(K.ip16(c["src"])), b"DstAddr": go_ip(K.ip16(c["dst"])), b"SrcPort": c["sport"], b"DstPort": c["dport"], b"Proto": c["proto"]}
    return dict(keys=keys, flows=c["flows"], bytes=c["bytes"], packets=c["packets"], start_min=c["start_min"], end_max=c["end_max"], first=values(c["first"]),
                last=values(c["last"]), hash=c["h"], type=c["rtype"].encode(), is_first=c["is_first"])
