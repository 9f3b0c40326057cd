#!/usr/bin/env python3
"""Validator.MatchBlob against SelectBlob for the same two claims and against
CheckBlob, in one process.

tools/paths_probe.py's pool and key set -- ES256 tokens signed for the 4 P-256
kids (tools/tokgen), served by a JWKS key set, with "scope", "roles" and
"realm_access":{"roles":[...]} added to every payload.  After one warm pass of
each entry three legs alternate for --passes timed passes each:

  match   MatchBlob([HasWord("scope", "write"), HasElement(Path("realm_access",
          "roles"), "uma_authorization"), HasWord("scope", "admin")]): a mask per
          token; the third requirement holds on no token of the pool
  select  SelectBlob(["scope", Path("realm_access", "roles")]): the columns a
          caller would search for the same two answers
  check   CheckBlob: the verdict alone

The medians, the ratios and the CAPJWT_TRACE phase laps of one more pass of each
are printed as one JSON line.  The three accept arrays must be identical, the
scan must have decided every token (host == 0), and the masks are checked
against the payloads of a sample of the pool.

  python tools/match_probe.py [--tokens 1048576] [--passes 5] [--kernels]

--kernels: instead of the three legs, three passes each of CheckBlobEach
(k_claims_scan_each), of the select leg (k_claims_paths_each) and of the match
leg (k_claims_match_each) on the same payloads, for a run under
`rocprofv3 --kernel-trace --stats`: the three kernels' times side by side in the
kernel statistics.
"""
import argparse
import array
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

# tools/paths_probe.py's extra members
EXTRA = '"roles":["admin","dev"],"scope":"read write","realm_access":{"roles":["offline_access","uma_authorization"]},'


def check_masks(pool, masks):
    """the masks of every 4099th token equal the two answers read from the payload"""
    n = len(pool)
    got = struct.unpack("<%dI" % n, masks)
    for i in range(0, n, 4099):
        seg = pool[i].split(b".")[1]
        claims = json.loads(base64.urlsafe_b64decode(seg + b"=" * (-len(seg) % 4)))
        want = int("write" in claims["scope"].split(" ")) | int("uma_authorization" in claims["realm_access"]["roles"]) << 1
        want |= int("admin" in claims["scope"].split(" ")) << 2
        assert got[i] == want, (i, got[i], want)
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    from cap_amd import jwt, _capjwt_host
    roles = jwt.Path("realm_access", "roles")
    # the third requirement never holds: the masks are not all ones
    requires = [jwt.HasWord("scope", "write"), jwt.HasElement(roles, "uma_authorization"), jwt.HasWord("scope", "admin")]
    names = ["scope", roles]
    threads = _capjwt_host.host_threads()
    kids = bench.E2E_KIDS
    os.environ["TOKGEN_EXTRA"] = EXTRA
    try:
        pool = bench.gen_tokens("ES256", args.tokens, bench.golden_keypaths(kids), threads, "pathsprobe")
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
    v.CheckBlob(b"\n".join(pool[:4096]), e)               # JWKS fetch + key staging
    ks.WaitTables()
    cstats, sstats, mstats = {}, {}, {}
    want = v.CheckBlob(blob, e, cstats)                   # one warm pass of each
    cols = v.SelectBlob(blob, names, e, sstats)
    assert cols["ok"] == want, "SelectBlob and CheckBlob verdicts differ"
    del cols
    cols = v.MatchBlob(blob, requires, e, mstats)
    assert cols["ok"] == want, "MatchBlob and CheckBlob verdicts differ"
    assert sum(want) == len(pool), f"accepted {sum(want)} of {len(pool)}"
    assert cstats == sstats == mstats == {"scanned": len(pool), "host": 0}, (cstats, sstats, mstats)
    masks = check_masks(pool, cols["match"])
    assert set(masks) == {3}, set(masks)
    del cols
    if args.kernels:
        which = array.array("I", bytes(4 * len(pool)))
        for _ in range(3):
            a = v.CheckBlobEach(blob, [e], which, cstats)
            b = v.SelectBlob(blob, names, e, sstats)
            c = v.MatchBlob(blob, requires, e, mstats)
            assert a == want and b["ok"] == want and c["ok"] == want
            assert cstats["host"] == 0 and sstats["host"] == 0 and mstats["host"] == 0
            del a, b, c
        print(json.dumps({"tokens": len(pool), "passes": 3,
                          "kernels": ["k_claims_scan_each", "k_claims_paths_each", "k_claims_match_each"]}))
        return
    t_chk, t_sel, t_mat = [], [], []
    for _ in range(args.passes):
        t0 = time.perf_counter()
        a = v.CheckBlob(blob, e, cstats)
        t1 = time.perf_counter()
        b = v.SelectBlob(blob, names, e, sstats)
        t2 = time.perf_counter()
        c = v.MatchBlob(blob, requires, e, mstats)
        t3 = time.perf_counter()
        assert a == want and b["ok"] == want and c["ok"] == want
        assert cstats["host"] == 0 and sstats["host"] == 0 and mstats["host"] == 0
        del b, c
        t_chk.append(t1 - t0)
        t_sel.append(t2 - t1)
        t_mat.append(t3 - t2)
    _, ph_chk = bench.with_trace_phases(lambda: v.CheckBlob(blob, e))
    _, ph_sel = bench.with_trace_phases(lambda: v.SelectBlob(blob, names, e))
    _, ph_mat = bench.with_trace_phases(lambda: v.MatchBlob(blob, requires, e))
    mc, ms, mm = statistics.median(t_chk), statistics.median(t_sel), statistics.median(t_mat)

    def leg(m, ts, ph):
        return {"tokens_per_s": len(pool) / m, "median_ms": m * 1e3, "all_ms": [t * 1e3 for t in ts], "phases_ms": ph}
    print(json.dumps({
        "tokens": len(pool), "passes": args.passes, "host_threads": threads,
        "payload_bytes": len(base64.urlsafe_b64decode(pool[0].split(b".")[1] + b"==")),
        "check_blob": leg(mc, t_chk, ph_chk), "select_blob": leg(ms, t_sel, ph_sel),
        "match_blob": dict(leg(mm, t_mat, ph_mat), scanned=mstats["scanned"], host=mstats["host"]),
        "match_over_select": ms / mm, "match_over_check": mc / mm}))


if __name__ == "__main__":
    main()
