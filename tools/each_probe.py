#!/usr/bin/env python3
"""Validator.CheckBlobEach against CheckBlob and against the split-by-tenant
workaround, in one process.

tools/check_probe.py's pool and key set -- ES256 tokens signed for the 4 P-256
kids (tools/tokgen), served by a JWKS key set -- generated once per profile
count P (TOKGEN_TENANTS=P): token i belongs to tenant i % P and carries that
tenant's issuer and audience, so every token is valid for its own profile and
for no other.  After one warm pass of each leg, the legs alternate for --passes
timed passes:

  check_blob        CheckBlob on the P = 1 pool with its one Expected (the baseline)
  each[P]           CheckBlobEach on the P pool, which[i] = i % P
  split[P]          what a caller does without it: the P pool cut into one blob
                    per tenant beforehand, P CheckBlob calls (the cutting and the
                    scatter back are not timed)

The medians, all laps, the ratios and the CAPJWT_TRACE phase laps of one more
pass of CheckBlob and of each[P] are printed as one JSON line.  Every leg must
accept every token with the scan deciding all of them (host == 0), and a
CheckBlobEach with the profiles rotated by one must reject every token (P > 1).

  python tools/each_probe.py [--tokens 1048576] [--passes 5] [--profiles 1,8,64]

The kernels' own times: run this under `rocprofv3 --kernel-trace --stats`
(k_claims_scan against k_claims_scan_each in the kernel statistics; --no-split
leaves the workaround's P small launches out of them).
"""
import argparse
import array
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the pool and the phase-lap parser of the end-to-end leg)

NOW = 1611699344 + 60


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--profiles", default="1,8,64")
    ap.add_argument("--no-split", action="store_true")
    args = ap.parse_args()
    counts = [int(x) for x in args.profiles.split(",")]
    if 1 not in counts:
        counts = [1] + counts
    from cap_amd import jwt, _capjwt_host
    threads = _capjwt_host.host_threads()
    kids = bench.E2E_KIDS
    jwk = [{"kty": "EC", "kid": f"kid-{i:02d}", "crv": "P-256", **xy} for i, xy in enumerate(bench.p256_jwk_xy(kids))]
    jwks = json.dumps({"keys": jwk}).encode()
    ks, err = jwt.NewJSONWebKeySet(None, "https://bench.example/jwks", "",
                                   lambda url, ca: {"status": 200, "body": jwks, "max_age": 3600})
    assert err is None, err
    v, _ = jwt.NewValidator(ks)

    def profile(p):
        return jwt.Expected(Issuer="https://t%02d.example/" % p, Audiences=["c%02d.example.com" % p],
                            SigningAlgorithms=["ES256"], Now=lambda: NOW)
    blobs, whichs, splits, profs = {}, {}, {}, {}
    payload_bytes = None
    for P in counts:
        os.environ["TOKGEN_TENANTS"] = str(P)
        try:
            pool = bench.gen_tokens("ES256", args.tokens, bench.golden_keypaths(kids), threads, "eachprobe%d" % P)
        finally:
            del os.environ["TOKGEN_TENANTS"]
        seg = pool[0].split(b".")[1]
        payload_bytes = len(seg) * 3 // 4
        blobs[P] = b"\n".join(pool)
        whichs[P] = array.array("I", [i % P for i in range(len(pool))])
        splits[P] = [b"\n".join(pool[p::P]) for p in range(P)]
        profs[P] = [profile(p) for p in range(P)]
        del pool
    n = args.tokens
    all_ok = bytes([1]) * n
    v.ValidateBlob(blobs[1][:400 * 4096].rsplit(b"\n", 1)[0], profs[1][0])       # JWKS fetch + key staging
    ks.WaitTables()

    def run_check():
        st = {}
        ok = v.CheckBlob(blobs[1], profs[1][0], st)
        assert ok == all_ok and st == {"scanned": n, "host": 0}, st

    def run_each(P):
        st = {}
        ok = v.CheckBlobEach(blobs[P], profs[P], whichs[P], st)
        assert ok == all_ok and st == {"scanned": n, "host": 0}, (P, st, sum(ok))

    def run_split(P):
        got = 0
        for p in range(P):
            st = {}
            ok = v.CheckBlob(splits[P][p], profs[P][p], st)
            assert st["host"] == 0
            got += sum(ok)
        assert got == n, (P, got)
    # one warm pass of each; the wrong tenant is a rejection
    assert v.ValidateBlob(blobs[1], profs[1][0]) == all_ok
    run_check()
    for P in counts:
        run_each(P)
        if not args.no_split:
            run_split(P)
        if P > 1:
            rot = profs[P][1:] + profs[P][:1]
            assert sum(v.CheckBlobEach(blobs[P], rot, whichs[P])) == 0, "a wrong-tenant token was accepted"
    laps = {"check_blob": []}
    for P in counts:
        laps["each_%d" % P] = []
        if not args.no_split:
            laps["split_%d" % P] = []

    def timed(name, fn, *a):
        t0 = time.perf_counter()
        fn(*a)
        laps[name].append(time.perf_counter() - t0)
    for _ in range(args.passes):
        timed("check_blob", run_check)
        for P in counts:
            timed("each_%d" % P, run_each, P)
            if not args.no_split:
                timed("split_%d" % P, run_split, P)
    phases = {"check_blob": bench.with_trace_phases(run_check)[1]}
    for P in counts:
        phases["each_%d" % P] = bench.with_trace_phases(lambda: run_each(P))[1]
    med = {k: statistics.median(t) for k, t in laps.items()}
    out = {"tokens": n, "passes": args.passes, "host_threads": threads, "profiles": counts,
           "payload_bytes": payload_bytes}
    for k, t in laps.items():
        out[k] = {"tokens_per_s": n / med[k], "median_ms": med[k] * 1e3, "all_ms": [x * 1e3 for x in t]}
        if k in phases:
            out[k]["phases_ms"] = phases[k]
    for P in counts:
        out["each_%d_over_check_blob" % P] = med["each_%d" % P] / med["check_blob"]
        if not args.no_split:
            out["split_%d_over_each_%d" % (P, P)] = med["split_%d" % P] / med["each_%d" % P]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
