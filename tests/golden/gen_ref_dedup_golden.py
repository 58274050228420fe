#!/usr/bin/env python3
"""Generates tests/golden/ref_dedup_golden.json: what the reference's own bpf/flows.c dedup merge (oracle/_ref/libref_flows.so,
`make -C oracle ref`) computes on the streams of tests/test_oracle_ref.py — the sha256 of its evictions per stream, the
aggregate its update_existing_flow leaves after the direct calls, and its observed-interface cut-off counter.

The library is built only where the reference checkout is readable and is git-ignored; these digests are committed so that
tests/test_oracle_ref.py pins the oracle to the reference in any checkout.

    make -C oracle ref && python tests/golden/gen_ref_dedup_golden.py      # rewrites tests/golden/ref_dedup_golden.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import test_oracle_ref as T          # noqa: E402  (the streams and the digest are defined once, there)
from oracle import oracle as O       # noqa: E402


def main():
    O.build()
    if not O.ref_available():
        raise SystemExit("oracle/_ref/libref_flows.so is not built: run `make -C oracle ref` where the reference checkout is readable")
    ref = O.ref_lib()
    out = {"what": "evictions of the reference's bpf/flows.c:76-143 merge (oracle/_ref/libref_flows.so) on the streams of "
                   "tests/test_oracle_ref.py: {evictions, flows, sha256 over every reason and record byte}",
           "streams": {}}
    for name, make in T.stream_cases(O).items():
        recs, m = make()
        if name == "missed_counter":
            ref.ref_counters_reset()
        out["streams"][name] = T.digest(O.run_ref_dedup(recs, m))
        if name == "missed_counter":
            out["missed_counter_observed_intf_missed"] = int(ref.ref_counter_observed_intf_missed())
    recs, agg = T.direct_case(O)
    out["direct_metrics_hex"] = T.ref_direct(ref, recs, agg).tobytes().hex()
    with open(os.path.join(HERE, "ref_dedup_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
