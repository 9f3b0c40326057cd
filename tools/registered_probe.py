#!/usr/bin/env python3
"""Validator.RegisteredBlob against ValidateBlob and CheckBlob in one process.

tools/check_probe.py's pool and key set: ES256 tokens signed for the 4 P-256
kids (tools/tokgen), served by a JWKS key set.  After one warm pass of each
entry the three alternate for --passes timed passes each; the medians, the
ratios and the CAPJWT_TRACE phase laps of one more pass of each are printed as
one JSON line.  The three accept arrays must be identical, the scan must have
decided every token (host == 0), and RegisteredBlob's sub / exp columns are
checked against the payloads of a sample of the pool.

  python tools/registered_probe.py [--tokens 1048576] [--passes 5]

The kernels' own times: run this under `rocprofv3 --kernel-trace --stats`
(k_claims_extract against k_claims_scan in the kernel statistics).
"""
import argparse
import base64
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the pool and the phase-lap parser of the end-to-end leg)


def check_columns(pool, cols):
    """sub and exp of every 4099th token, from the columns, equal the payload's"""
    n = len(pool)
    off, data = cols["sub"]
    off = struct.unpack("<%dI" % (n + 1), off)
    exp = struct.unpack("<%dq" % n, cols["exp"])
    for i in range(0, n, 4099):
        seg = pool[i].split(b".")[1]
        claims = json.loads(base64.urlsafe_b64decode(seg + b"=" * (-len(seg) % 4)))
        assert data[off[i]:off[i + 1]].decode() == claims.get("sub", ""), (i, claims)
        assert exp[i] == claims.get("exp", 0) and (cols["present"][i] >> 5) & 1 == int("exp" in claims), (i, claims)


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
    stats, rstats = {}, {}
    assert v.CheckBlob(blob, e, stats) == want, "CheckBlob and ValidateBlob verdicts differ"
    cols = v.RegisteredBlob(blob, e, rstats)
    assert cols["ok"] == want, "RegisteredBlob and ValidateBlob verdicts differ"
    assert sum(want) == len(pool), f"accepted {sum(want)} of {len(pool)}"
    assert stats == rstats == {"scanned": len(pool), "host": 0}, (stats, rstats)
    check_columns(pool, cols)
    del cols
    t_val, t_chk, t_reg = [], [], []
    for _ in range(args.passes):
        t0 = time.perf_counter()
        a = v.ValidateBlob(blob, e)
        t1 = time.perf_counter()
        b = v.CheckBlob(blob, e, stats)
        t2 = time.perf_counter()
        c = v.RegisteredBlob(blob, e, rstats)
        t3 = time.perf_counter()
        assert a == want and b == want and c["ok"] == want and stats["host"] == 0 and rstats["host"] == 0
        del c
        t_val.append(t1 - t0)
        t_chk.append(t2 - t1)
        t_reg.append(t3 - t2)
    _, ph_val = bench.with_trace_phases(lambda: v.ValidateBlob(blob, e))
    _, ph_chk = bench.with_trace_phases(lambda: v.CheckBlob(blob, e))
    _, ph_reg = bench.with_trace_phases(lambda: v.RegisteredBlob(blob, e))
    mv, mc, mr = statistics.median(t_val), statistics.median(t_chk), statistics.median(t_reg)

    def leg(m, ts, ph):
        return {"tokens_per_s": len(pool) / m, "median_ms": m * 1e3, "all_ms": [t * 1e3 for t in ts], "phases_ms": ph}
    print(json.dumps({
        "tokens": len(pool), "passes": args.passes, "host_threads": threads,
        "validate_blob": leg(mv, t_val, ph_val), "check_blob": leg(mc, t_chk, ph_chk),
        "registered_blob": dict(leg(mr, t_reg, ph_reg), scanned=rstats["scanned"], host=rstats["host"]),
        "registered_over_validate": mv / mr, "check_over_registered": mr / mc}))


if __name__ == "__main__":
    main()
