"""Independent restatement of the direct-FLP stdout line with its TLS keys, for the tests (no import of the product): the
maps of tests/flp_json_ref.py, flp_json_content_ref.py and netev_ref.py, without their is_deferred gate, plus

  pkg/decode/decode_protobuf.go:99-110   TLSVersion, TLSCipherSuite, TLSGroup (TLSTypes is in flp_json_ref already)
  pkg/model/record.go:240-257            SSLVersionToString: "~ " in front when MiscFlagsSSLMismatch (misc_flags & 1) is set

The names are not restated here either: they come in as a table {(kind, id): name bytes}, kind 0 = version, 1 = cipher
suite, 2 = group. An id without a name prints as Go's crypto/tls prints an unknown value: 0x%04X for a version or a cipher
suite, CurveID(%d) for a group."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flp_json_content_ref as RC  # noqa: E402
import netev_ref as RN  # noqa: E402
from flp_json_ref import _METRICS, jsoniter_string, marshal_sorted, record_to_map  # noqa: E402

VERSION, CIPHER_SUITE, GROUP = 0, 1, 2
MISMATCH = 0x01


def table_of(entries) -> dict:
    """[(kind, id, name str or bytes)] -> {(kind, id): bytes}."""
    return {(k, i): n.encode() if isinstance(n, str) else bytes(n) for k, i, n in entries}


def render(names: dict, kind: int, ident: int, mismatch: bool = False) -> bytes:
    if not 0 <= ident <= 0xFFFF:
        raise ValueError("the record's fields are 16 bits wide")
    v = names.get((kind, ident))
    if v is None:
        v = b"CurveID(%d)" % ident if kind == GROUP else b"0x%04X" % ident
    return b"~ " + v if kind == VERSION and mismatch else v


def add_tls(out: dict, rec: bytes, names: dict) -> dict:
    m = _METRICS.unpack_from(rec, 40)
    ssl, cipher, share, misc = m[22], m[23], m[24], m[26]
    if ssl:
        out[b"TLSVersion"] = render(names, VERSION, ssl, bool(misc & MISMATCH))
    if cipher:
        out[b"TLSCipherSuite"] = render(names, CIPHER_SUITE, cipher)
    if share:
        out[b"TLSGroup"] = render(names, GROUP, share)
    return out


def encode(records, names_tls: dict, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown=b"unknown", present=None, parts=None,
           events=None):
    """The lines of these flows, none deferred. present / parts: the content policy (flp_json_content_ref.encode); events (per
    flow the decoder's answers, netev_ref.resolve's fourth result, present / parts["drops"] its first two): the network-events
    policy. Returns (bytes, offsets uint64[n + 1])."""
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1, 144)
    n = len(raw)
    off = np.zeros(n + 1, dtype=np.uint64)
    memo, lines, pos = {}, [], 0
    for i in range(n):
        rec = raw[i].tobytes()
        m = add_tls(record_to_map(rec, now_unix_ns, mono_now_ns, names, agent_ip, time_received, unknown, memo), rec, names_tls)
        if present is not None:
            RC.add_content(m, RC.flow_parts(present, parts, i))
        body = marshal_sorted(m)
        if events is not None and events[i]:                # spliced in as netev_ref.encode_json does
            keys = sorted(list(m) + [b"NetworkEvents"])
            at = keys.index(b"NetworkEvents")
            val = b'"NetworkEvents":[' + b",".join(RN.render_json(e) for e in events[i]) + b"]"
            head = marshal_sorted({k: m[k] for k in keys[:at]})[:-1]
            tail = marshal_sorted({k: m[k] for k in keys[at + 1:]})[1:]
            body = head + (b"," if at else b"") + val + (b"," if len(tail) > 1 else b"") + tail
        lines.append(body + b"\n")
        pos += len(lines[-1])
        off[i + 1] = pos
    return b"".join(lines), off


__all__ = ["VERSION", "CIPHER_SUITE", "GROUP", "table_of", "render", "add_tls", "encode", "jsoniter_string"]
