#!/usr/bin/env python3
"""Validator.SelectBlob against ValidateBlob and RegisteredBlob in one process.

tools/registered_probe.py's pool and key set -- ES256 tokens signed for the 4
P-256 kids (tools/tokgen), served by a JWKS key set -- with two members added
to every payload: "scope" (a string) and "roles" (an array).  After one warm
pass of each entry the three alternate for --passes timed passes each; the
medians, the ratios and the CAPJWT_TRACE phase laps of one more pass of each
are printed as one JSON line.  The three accept arrays must be identical, the
scan must have decided every token (host == 0), and SelectBlob's scope / roles
columns are checked against the payloads of a sample of the pool.

  python tools/select_probe.py [--tokens 1048576] [--passes 5] [--names scope,roles]

The kernels' own times: run this under `rocprofv3 --kernel-trace --stats`
(k_claims_select against k_claims_extract in the kernel statistics).
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

EXTRA = '"roles":["admin","dev"],"scope":"read write",'


def check_columns(pool, names, cols):
    """the selected values of every 4099th token, from the columns, equal the payload's"""
    n = len(pool)
    for name, c in zip(names, cols["sel"]):
        off = struct.unpack("<%dI" % (n + 1), c["text_off"])
        for i in range(0, n, 4099):
            seg = pool[i].split(b".")[1]
            claims = json.loads(base64.urlsafe_b64decode(seg + b"=" * (-len(seg) % 4)))
            text = c["text"][off[i]:off[i + 1]]
            want = claims.get(name)
            if isinstance(want, str):
                assert c["type"][i] == 1 and text.decode() == want, (i, name, text)
            elif isinstance(want, (list, dict)):
                assert c["type"][i] in (7, 8) and json.loads(text) == want, (i, name, text)
            else:
                assert (c["type"][i] == 0) == (name not in claims) and text == b"", (i, name, text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--names", default="scope,roles")
    args = ap.parse_args()
    names = [x for x in args.names.split(",") if x]
    from cap_amd import jwt, _capjwt_host
    threads = _capjwt_host.host_threads()
    kids = bench.E2E_KIDS
    os.environ["TOKGEN_EXTRA"] = EXTRA
    try:
        pool = bench.gen_tokens("ES256", args.tokens, bench.golden_keypaths(kids), threads, "selectprobe")
    finally:
        del os.environ["TOKGEN_EXTRA"]
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
    rstats, sstats = {}, {}
    cols = v.RegisteredBlob(blob, e, rstats)
    assert cols["ok"] == want, "RegisteredBlob and ValidateBlob verdicts differ"
    reg_sub = cols["sub"]
    cols = v.SelectBlob(blob, names, e, sstats)
    assert cols["ok"] == want, "SelectBlob and ValidateBlob verdicts differ"
    assert cols["sub"] == reg_sub, "SelectBlob's and RegisteredBlob's sub columns differ"
    assert sum(want) == len(pool), f"accepted {sum(want)} of {len(pool)}"
    assert rstats == sstats == {"scanned": len(pool), "host": 0}, (rstats, sstats)
    check_columns(pool, names, cols)
    del cols, reg_sub
    t_val, t_reg, t_sel = [], [], []
    for _ in range(args.passes):
        t0 = time.perf_counter()
        a = v.ValidateBlob(blob, e)
        t1 = time.perf_counter()
        b = v.RegisteredBlob(blob, e, rstats)
        t2 = time.perf_counter()
        c = v.SelectBlob(blob, names, e, sstats)
        t3 = time.perf_counter()
        assert a == want and b["ok"] == want and c["ok"] == want and rstats["host"] == 0 and sstats["host"] == 0
        del b, c
        t_val.append(t1 - t0)
        t_reg.append(t2 - t1)
        t_sel.append(t3 - t2)
    _, ph_val = bench.with_trace_phases(lambda: v.ValidateBlob(blob, e))
    _, ph_reg = bench.with_trace_phases(lambda: v.RegisteredBlob(blob, e))
    _, ph_sel = bench.with_trace_phases(lambda: v.SelectBlob(blob, names, e))
    mv, mr, ms = statistics.median(t_val), statistics.median(t_reg), statistics.median(t_sel)

    def leg(m, ts, ph):
        return {"tokens_per_s": len(pool) / m, "median_ms": m * 1e3, "all_ms": [t * 1e3 for t in ts], "phases_ms": ph}
    print(json.dumps({
        "tokens": len(pool), "passes": args.passes, "host_threads": threads, "names": names,
        "payload_bytes": len(base64.urlsafe_b64decode(pool[0].split(b".")[1] + b"==")),
        "validate_blob": leg(mv, t_val, ph_val), "registered_blob": leg(mr, t_reg, ph_reg),
        "select_blob": dict(leg(ms, t_sel, ph_sel), scanned=sstats["scanned"], host=sstats["host"]),
        "select_over_validate": mv / ms, "registered_over_select": ms / mr}))


if __name__ == "__main__":
    main()
