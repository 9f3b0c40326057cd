#!/usr/bin/env python3
"""Validator.MatchBlobArgs -- a nonce and an auth_time bound per token -- against
MatchBlob with two constant predicates, CheckBlob, and the workaround it
replaces (SelectBlob of the two claims plus the comparison in Python), in one
process.

tools/match_probe.py's pool and key set -- ES256 tokens signed for the 4 P-256
kids (tools/tokgen), served by a JWKS key set -- with a distinct 22-byte "nonce"
and an integer "auth_time" in every payload (TOKGEN_OIDC).  After one warm pass
of each entry four legs alternate for --passes timed passes each:

  args    MatchBlobArgs([EqualsEach("nonce", 0), AtLeastEach("auth_time", 0)]):
          the request's nonce and its auth_time bound travel as columns, a mask
          per token comes back
  match   MatchBlob([Equals("nonce", <token 0's>), Present("auth_time")]): two
          constant predicates, no operand upload
  check   CheckBlob: the verdict alone
  select  the workaround: SelectBlob(["nonce", "auth_time"]) and the two
          comparisons in Python over its columns

The medians, the five laps of each, the ratios and the CAPJWT_TRACE phase laps of
one more pass are printed as one JSON line.  The accept arrays must be identical,
the scan must have decided every token (host == 0), the workaround's answers must
equal the masks, and every fourth operand is wrong, so the masks are not all ones.

  python tools/match_args_probe.py [--tokens 1048576] [--passes 5] [--kernels]

--kernels: instead of the legs, three passes each of the match leg
(k_claims_match_each) and of the args leg (k_claims_match_args) on the same
payloads, for a run under `rocprofv3 --kernel-trace --stats`: the two kernels'
times side by side in the kernel statistics.
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

T0 = 1611699344
SEL_STRING, SEL_NUMBER = 1, 3                             # jg_sel_type


def nonce_of(i):
    return b"n-%020x" % i                                  # tools/tokgen, TOKGEN_OIDC


def auth_of(i):
    return T0 - i % 3600


def operands(n):
    """The requests' side: the nonce each token was issued for, wrong for every fourth token, and the earliest
    auth_time each request takes (max_age 1800 s before T0)"""
    nonces = [nonce_of(i if i % 4 != 3 else i + 1) for i in range(n)]
    bounds = array.array("q", [T0 - 1800]) * n
    return nonces, bounds


def want_masks(n):
    return [int(i % 4 != 3) | int(auth_of(i) >= T0 - 1800) << 1 for i in range(n)]


def workaround(v, blob, e, nonces, bounds, stats=None):
    """SelectBlob of the two claims and the comparisons in Python -> (ok, masks)"""
    cols = v.SelectBlob(blob, ["nonce", "auth_time"], e, stats)
    n = len(nonces)
    c0, c1 = cols["sel"]
    off = struct.unpack("<%dI" % (n + 1), c0["text_off"])
    text, t0, t1 = c0["text"], c0["type"], c1["type"]
    num = struct.unpack("<%dd" % n, c1["num"])
    masks = [int(t0[i] == SEL_STRING and text[off[i]:off[i + 1]] == nonces[i])
             | int(t1[i] == SEL_NUMBER and num[i] >= float(bounds[i])) << 1 for i in range(n)]
    return cols["ok"], masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    from cap_amd import jwt, _capjwt_host
    threads = _capjwt_host.host_threads()
    kids = bench.E2E_KIDS
    os.environ["TOKGEN_OIDC"] = "1"
    try:
        pool = bench.gen_tokens("ES256", args.tokens, bench.golden_keypaths(kids), threads, "argsprobe")
    finally:
        del os.environ["TOKGEN_OIDC"]
    n = len(pool)
    seg = pool[5].split(b".")[1]
    first = json.loads(base64.urlsafe_b64decode(seg + b"=" * (-len(seg) % 4)))
    assert first["nonce"].encode() == nonce_of(5) and first["auth_time"] == auth_of(5), "tools/tokgen is stale: rebuild it"
    jwk = [{"kty": "EC", "kid": f"kid-{i:02d}", "crv": "P-256", **xy} for i, xy in enumerate(bench.p256_jwk_xy(kids))]
    jwks = json.dumps({"keys": jwk}).encode()
    ks, err = jwt.NewJSONWebKeySet(None, "https://bench.example/jwks", "",
                                   lambda url, ca: {"status": 200, "body": jwks, "max_age": 3600})
    assert err is None, err
    v, _ = jwt.NewValidator(ks)
    e = jwt.Expected(Issuer="https://example.com/", Audiences=["www.example.com"], SigningAlgorithms=["ES256"],
                     Now=lambda: T0 + 60)
    requires = [jwt.EqualsEach("nonce", 0), jwt.AtLeastEach("auth_time", 0)]
    constant = [jwt.Equals("nonce", nonce_of(0).decode()), jwt.Present("auth_time")]
    nonces, bounds = operands(n)
    ncol = b"\n".join(nonces)
    blob = b"\n".join(pool)
    v.CheckBlob(b"\n".join(pool[:4096]), e)               # JWKS fetch + key staging
    ks.WaitTables()
    cstats, sstats, mstats, astats = {}, {}, {}, {}
    want = v.CheckBlob(blob, e, cstats)                   # one warm pass of each
    ok, smasks = workaround(v, blob, e, nonces, bounds, sstats)
    assert ok == want, "SelectBlob and CheckBlob verdicts differ"
    cols = v.MatchBlob(blob, constant, e, mstats)
    assert cols["ok"] == want, "MatchBlob and CheckBlob verdicts differ"
    cols = v.MatchBlobArgs(blob, requires, [ncol], [bounds], e, astats)
    assert cols["ok"] == want, "MatchBlobArgs and CheckBlob verdicts differ"
    assert sum(want) == n, f"accepted {sum(want)} of {n}"
    assert cstats == sstats == mstats == astats == {"scanned": n, "host": 0}, (cstats, sstats, mstats, astats)
    masks = list(struct.unpack("<%dI" % n, cols["match"]))
    assert masks == smasks == want_masks(n), "the masks differ from the workaround's or from the pool's"
    assert set(masks) == {0, 1, 2, 3} or n < 8192, set(masks)
    del cols
    if args.kernels:
        for _ in range(3):
            a = v.MatchBlob(blob, constant, e, mstats)
            b = v.MatchBlobArgs(blob, requires, [ncol], [bounds], e, astats)
            assert a["ok"] == want and b["ok"] == want and mstats["host"] == 0 and astats["host"] == 0
            del a, b
        print(json.dumps({"tokens": n, "passes": 3, "kernels": ["k_claims_match_each", "k_claims_match_args"]}))
        return
    t = {"args": [], "match": [], "check": [], "select": []}
    for _ in range(args.passes):
        t0 = time.perf_counter()
        a = v.MatchBlobArgs(blob, requires, [ncol], [bounds], e, astats)
        t1 = time.perf_counter()
        b = v.MatchBlob(blob, constant, e, mstats)
        t2 = time.perf_counter()
        c = v.CheckBlob(blob, e, cstats)
        t3 = time.perf_counter()
        d, dm = workaround(v, blob, e, nonces, bounds, sstats)
        t4 = time.perf_counter()
        assert a["ok"] == want and b["ok"] == want and c == want and d == want
        assert astats["host"] == 0 and mstats["host"] == 0 and cstats["host"] == 0 and sstats["host"] == 0
        assert a["match"] == struct.pack("<%dI" % n, *dm)
        del a, b, c, d, dm
        for name, dt in zip(("args", "match", "check", "select"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            t[name].append(dt)
    _, ph_args = bench.with_trace_phases(lambda: v.MatchBlobArgs(blob, requires, [ncol], [bounds], e))
    _, ph_mat = bench.with_trace_phases(lambda: v.MatchBlob(blob, constant, e))
    med = {k: statistics.median(x) for k, x in t.items()}

    def leg(name, ph=None):
        out = {"tokens_per_s": n / med[name], "median_ms": med[name] * 1e3, "all_ms": [x * 1e3 for x in t[name]]}
        if ph is not None:
            out["phases_ms"] = ph
        return out
    print(json.dumps({
        "tokens": n, "passes": args.passes, "host_threads": threads,
        "payload_bytes": len(base64.urlsafe_b64decode(pool[0].split(b".")[1] + b"==")),
        "operand_bytes_per_token": 8 + len(nonces[0]) + 8,
        "match_blob_args": dict(leg("args", ph_args), scanned=astats["scanned"], host=astats["host"]),
        "match_blob": leg("match", ph_mat), "check_blob": leg("check"), "select_blob_plus_python": leg("select"),
        "args_over_workaround": med["select"] / med["args"], "args_over_match": med["match"] / med["args"],
        "args_over_check": med["check"] / med["args"],
        # the acceptance condition: faster than the workaround by more than the spread of the five laps
        "slowest_args_ms": max(t["args"]) * 1e3, "fastest_workaround_ms": min(t["select"]) * 1e3,
        "beats_workaround_beyond_spread": max(t["args"]) < min(t["select"])}))


if __name__ == "__main__":
    main()
