#!/usr/bin/env python3
"""Validator.CheckBlob against Validator.ValidateBlob in one process.

The pool is the one bench.py's end-to-end leg builds: ES256 tokens signed for
the 4 P-256 kids (tools/tokgen), served by a JWKS key set.  After one warm pass
of each entry the two alternate for --passes timed passes each; the medians,
their ratio and the CAPJWT_TRACE phase laps of one more pass of each are
printed as one JSON line.  The two verdict arrays must be identical and the
claims scan must have decided every token (host == 0).

  python tools/check_probe.py [--tokens 1048576] [--passes 5]

The scan kernel's own time: run this under `rocprofv3 --kernel-trace --stats`
(k_claims_scan in the kernel statistics).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the pool and the phase-lap parser of the end-to-end leg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 20)
    ap.add_argument("--passes", type=int, default=5)
    args = ap.parse_args()
    from cap_amd import jwt, _capjwt_host
    threads = _capjwt_host.host_threads()
    kids = bench.E2E_KIDS
    pool = bench.gen_tokens("ES256", args.tokens, bench.golden_keypaths(kids), threads, "checkprobe")
    jwk = [{"kty": "EC", "kid": f"kid-{i:02d}", "crv": "P-256", **xy} for i, xy in enumerate(bench.p256_jwk_xy(kids))]
    jwks = json.dumps({"keys": jwk}).encode()
    ks, err = jwt.NewJSONWebKeySet(None, "https://bench.example/jwks", "",
                                   lambda url, ca: {"status": 200, "body": jwks, "max_age": 3600})
    assert err is None, err
    v, _ = jwt.NewValidator(ks)
    e = jwt.Expected(Issuer="https://example.com/", Audiences=["www.example.com"], SigningAlgorithms=["ES256"],
                     Now=lambda: 1611699344 + 60)
    blob = b"\n".join(pool)
    v.ValidateBlob(b"\n".join(pool[:4096]), e)           # JWKS fetch + key staging
    ks.WaitTables()
    want = v.ValidateBlob(blob, e)                        # one warm pass of each
    stats = {}
    got = v.CheckBlob(blob, e, stats)
    assert got == want, "CheckBlob and ValidateBlob verdicts differ"
    assert sum(want) == len(pool), f"accepted {sum(want)} of {len(pool)}"
    assert stats == {"scanned": len(pool), "host": 0}, stats
    t_val, t_chk = [], []
    for _ in range(args.passes):
        t0 = time.perf_counter()
        a = v.ValidateBlob(blob, e)
        t1 = time.perf_counter()
        b = v.CheckBlob(blob, e, stats)
        t2 = time.perf_counter()
        assert a == want and b == want and stats["host"] == 0
        t_val.append(t1 - t0)
        t_chk.append(t2 - t1)
    _, ph_val = bench.with_trace_phases(lambda: v.ValidateBlob(blob, e))
    _, ph_chk = bench.with_trace_phases(lambda: v.CheckBlob(blob, e))
    mv, mc = statistics.median(t_val), statistics.median(t_chk)
    print(json.dumps({
        "tokens": len(pool), "passes": args.passes, "host_threads": threads,
        "validate_blob": {"tokens_per_s": len(pool) / mv, "median_ms": mv * 1e3, "all_ms": [t * 1e3 for t in t_val],
                          "phases_ms": ph_val},
        "check_blob": {"tokens_per_s": len(pool) / mc, "median_ms": mc * 1e3, "all_ms": [t * 1e3 for t in t_chk],
                       "phases_ms": ph_chk, "scanned": stats["scanned"], "host": stats["host"]},
        "check_over_validate": mv / mc}))
    assert mc < mv, "CheckBlob's median is not above ValidateBlob's"


if __name__ == "__main__":
    main()
