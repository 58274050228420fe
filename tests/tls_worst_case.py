"""The flow whose direct-FLP line with TLS names is the longest one each policy can write (0: records only, 1: with every
feature part, 2: with four network events as well), for tests/test_flp_json_tls_cpu.py and test_flp_json_tls_gpu.py: every
key present, every number at its widest, seven interfaces whose 16-byte names and 63-byte UDNs escape six-fold, a
31-byte DNS name that escapes six-fold, three TLS names of 63 bytes behind the mismatch mark, four events whose objects
render to 512 bytes. `nf` is passed in for the record layouts only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_tls_ref as T  # noqa: E402
import netev_ref as RN  # noqa: E402

V6 = bytes.fromhex("1111222233334444555566667777888f")          # no zero group, four digits each: 39 characters
NAMES = [(7, None, b"\x01" * 16, b"\x02" * 63)]
TLS = [(T.VERSION, 0xFFFE, "V" * 63), (T.CIPHER_SUITE, 0xFFFE, "C" * 63), (T.GROUP, 0xFFFE, "G" * 63)]
# time.Time.Add over the two most distant int64 nanosecond counts: -18446744073.9 s, 15 characters as milliseconds
NOW, MONO, RECEIVED = -2**63, 2**63 - 1, -2**62
EVENT_BYTES = 512


def worst_case(nf, n, policy):
    recs = np.zeros(n, dtype=nf.FLOW_RECORD)
    k, m = recs["id"], recs["metrics"]
    k["src_ip"] = k["dst_ip"] = np.frombuffer(V6, dtype=np.uint8)
    k["src_port"] = k["dst_port"] = 65535
    k["transport_protocol"] = 6
    m["eth_protocol"], m["if_index_first_seen"], m["nb_observed_intf"], m["observed_intf"] = 0x86DD, 7, 6, 7
    m["direction_first_seen"], m["observed_direction"] = 255, 255
    m["bytes"], m["packets"], m["sampling"], m["dscp"], m["flags"], m["tls_types"] = 2**64 - 1, 2**32 - 1, 2**32 - 1, 255, 65535, 63
    m["src_mac"] = m["dst_mac"] = 0xAB
    m["ssl_version"] = m["tls_cipher_suite"] = m["tls_key_share"] = 0xFFFE
    m["misc_flags"] = 1
    case = dict(recs=recs, present=None, parts=None, answers=None, names=NAMES, tls=TLS, now=NOW, mono=MONO, agent=V6, received=RECEIVED)
    if policy == 0:
        return case
    parts = {kind: np.zeros(n, dtype=nf.ROLLUP_KINDS[kind]) for kind in ("additional", "dns", "drops", "xlat", "quic", "network_events")}
    d, p, x, a, q = (parts[kind] for kind in ("dns", "drops", "xlat", "additional", "quic"))
    d["id"], d["flags"], d["errno_"], d["latency"] = 65535, 0xFFFB, 255, 2**63
    d["name"] = np.frombuffer(b"\x1f" + b"\x01" * 31, dtype=np.uint8)
    p["bytes"], p["packets"], p["latest_flags"], p["latest_state"], p["latest_drop_cause"] = 65535, 65535, 65535, 0, 13
    x["saddr"] = x["daddr"] = np.frombuffer(V6, dtype=np.uint8)
    x["sport"], x["dport"], x["zone_id"] = 65535, 65535, 65535
    a["ipsec_encrypted_ret"], a["flow_rtt"] = -2**31, 2**63
    q["version"], q["seen_long_hdr"], q["seen_short_hdr"] = 0xFFFFFFFF, 255, 255
    case["present"] = np.full(n, 0x37, dtype=np.uint8)
    case["parts"] = parts
    if policy == 2:
        # one escaped quote: the JSON object and the protobuf message both have exactly 512 bytes, the cap of either rendering
        answers = {bytes([c + 1] * 8): b'"' + bytes([0x41 + c]) * (EVENT_BYTES - len(b'{"Message":"\\""}')) for c in range(4)}
        ne = parts["network_events"]
        for c, cookie in enumerate(answers):
            ne["network_events"][:, c] = np.frombuffer(cookie, dtype=np.uint8)
        ne["packets"], ne["bytes"] = 1, 1
        case["present"] |= 8
        case["answers"] = answers
    return case


def reference(case):
    """(bytes, offsets) of the restatement for a case of worst_case()."""
    present, parts, events = case["present"], case["parts"], None
    if case["answers"] is not None:
        present, drops, _rows, events, missing = RN.resolve(present, parts["network_events"], parts["drops"], case["answers"])
        assert not missing and all(len(e) == 4 for e in events) and all(len(RN.render_json(v)) == EVENT_BYTES for v in case["answers"].values())
        parts = {**parts, "drops": drops.view(parts["drops"].dtype).reshape(-1)}
    return T.encode(case["recs"], T.table_of(case["tls"]), case["now"], case["mono"], case["names"], case["agent"], case["received"],
                    present=present, parts=parts, events=events)
