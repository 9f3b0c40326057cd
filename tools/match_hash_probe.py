#!/usr/bin/env python3
"""Validator.MatchBlobArgs with a hash column -- the request's nonce and its
access token against at_hash, in one call -- against the nonce alone and against
the workaround it replaces (MatchBlobArgs for the nonce, then
oidc.VerifyAccessTokenBatch for at_hash), in one process.

tools/match_args_probe.py's pool and key set -- ES256 tokens signed for the 4
P-256 kids (tools/tokgen), served by a JWKS key set -- with a distinct 22-byte
"nonce", an integer "auth_time" and the "at_hash" of a distinct 40-byte access
token in every payload (TOKGEN_OIDC=2).  After one warm pass of each, three legs
alternate for --passes timed passes each:

  nonce   MatchBlobArgs([EqualsEach("nonce", 0)])
  hash    MatchBlobArgs([EqualsEach("nonce", 0), HashOfEach("at_hash", 0), IsString("at_hash")],
          hashes=[access tokens]): the new call
  two     the workaround: the nonce leg, then oidc.VerifyAccessTokenBatch(tokens, access tokens)

Every fourth nonce and every fifth access token is wrong, so the masks are not all
ones; the new call's bits must equal the workaround's answers.  The medians, the
laps of each, the lap spreads and the ratios are printed as one JSON line and
written to --out (default profiles/match_hash.json).

  python tools/match_hash_probe.py [--tokens 1048576] [--passes 5] [--out FILE] [--kernels]

--kernels: instead of the legs, three passes each of the nonce leg and of the hash
leg on the same payloads, for a run under `rocprofv3 --kernel-trace --stats`:
k_hash_operand and k_claims_match_args side by side in the kernel statistics.
With --parent the tool runs the nonce leg alone on match_args_probe.py's payloads
(what the parent commit has too: copy this file into a build of it), so that
k_claims_match_args' time there can be set beside this commit's.
"""
import argparse
import base64
import hashlib
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the pool of the end-to-end leg)

T0 = 1611699344


def nonce_of(i):
    return b"n-%020x" % i                                  # tools/tokgen, TOKGEN_OIDC


def access_token_of(i):
    return b"ya29.%035x" % i                               # tools/tokgen, TOKGEN_OIDC=2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_hash.json"))
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--parent", action="store_true")
    args = ap.parse_args()
    from cap_amd import jwt, oidc, _capjwt_host
    threads = _capjwt_host.host_threads()
    kids = bench.E2E_KIDS
    os.environ["TOKGEN_OIDC"] = "1" if args.parent else "2"   # --parent: the payloads both commits can make
    try:
        pool = bench.gen_tokens("ES256", args.tokens, bench.golden_keypaths(kids), threads, "hashprobe")
    finally:
        del os.environ["TOKGEN_OIDC"]
    n = len(pool)
    seg = pool[5].split(b".")[1]
    first = json.loads(base64.urlsafe_b64decode(seg + b"=" * (-len(seg) % 4)))
    want_at = base64.urlsafe_b64encode(hashlib.sha256(access_token_of(5)).digest()[:16]).rstrip(b"=").decode()
    assert first["nonce"].encode() == nonce_of(5) and (args.parent or first.get("at_hash") == want_at), \
        "tools/tokgen is stale: rebuild it"
    jwk = [{"kty": "EC", "kid": f"kid-{i:02d}", "crv": "P-256", **xy} for i, xy in enumerate(bench.p256_jwk_xy(kids))]
    jwks = json.dumps({"keys": jwk}).encode()
    ks, err = jwt.NewJSONWebKeySet(None, "https://bench.example/jwks", "",
                                   lambda url, ca: {"status": 200, "body": jwks, "max_age": 3600})
    assert err is None, err
    v, _ = jwt.NewValidator(ks)
    e = jwt.Expected(Issuer="https://example.com/", Audiences=["www.example.com"], SigningAlgorithms=["ES256"],
                     Now=lambda: T0 + 60)
    nonce_req = [jwt.EqualsEach("nonce", 0)]
    nonces = [nonce_of(i if i % 4 != 3 else i + 1) for i in range(n)]
    ats = [access_token_of(i if i % 5 != 4 else i + 1) for i in range(n)]
    ncol, acol = b"\n".join(nonces), b"\n".join(ats)
    blob = b"\n".join(pool)
    toks = [t.decode() for t in pool]
    v.CheckBlob(b"\n".join(pool[:4096]), e)               # JWKS fetch + key staging
    ks.WaitTables()
    nstats, hstats = {}, {}
    want = v.CheckBlob(blob, e)
    cols = v.MatchBlobArgs(blob, nonce_req, [ncol], [], e, nstats)
    assert cols["ok"] == want and sum(want) == n and nstats == {"scanned": n, "host": 0}, nstats
    nmasks = list(struct.unpack("<%dI" % n, cols["match"]))
    assert nmasks == [int(i % 4 != 3) for i in range(n)]
    if args.parent:
        for _ in range(3):
            v.MatchBlobArgs(blob, nonce_req, [ncol], [], e, nstats)
        print(json.dumps({"tokens": n, "passes": 4, "kernels": ["k_claims_match_args"], "leg": "nonce"}))
        return
    hash_req = nonce_req + [jwt.HashOfEach("at_hash", 0), jwt.IsString("at_hash")]
    cols = v.MatchBlobArgs(blob, hash_req, [ncol], [], e, hstats, hashes=[acol])
    assert cols["ok"] == want and hstats == {"scanned": n, "host": 0}, hstats
    hmasks = list(struct.unpack("<%dI" % n, cols["match"]))
    assert hmasks == [int(i % 4 != 3) | int(i % 5 != 4) << 1 | 4 for i in range(n)], "the masks differ from the pool's"
    res = oidc.VerifyAccessTokenBatch(toks, ats)           # the workaround's second pass
    assert [bool(r[0]) for r in res] == [bool(m & 2) for m in hmasks], "VerifyAccessTokenBatch disagrees with the masks"
    del cols, res
    if args.kernels:
        for _ in range(3):
            v.MatchBlobArgs(blob, nonce_req, [ncol], [], e, nstats)
            v.MatchBlobArgs(blob, hash_req, [ncol], [], e, hstats, hashes=[acol])
        print(json.dumps({"tokens": n, "passes": 3, "kernels": ["k_hash_operand", "k_claims_match_args"]}))
        return
    t = {"nonce": [], "hash": [], "two": []}
    for _ in range(args.passes):
        t0 = time.perf_counter()
        a = v.MatchBlobArgs(blob, nonce_req, [ncol], [], e, nstats)
        t1 = time.perf_counter()
        b = v.MatchBlobArgs(blob, hash_req, [ncol], [], e, hstats, hashes=[acol])
        t2 = time.perf_counter()
        c = v.MatchBlobArgs(blob, nonce_req, [ncol], [], e, nstats)
        d = oidc.VerifyAccessTokenBatch(toks, ats)
        t3 = time.perf_counter()
        assert a["ok"] == want and b["ok"] == want and c["ok"] == want and nstats["host"] == 0 and hstats["host"] == 0
        assert len(d) == n
        del a, b, c, d
        for name, dt in zip(("nonce", "hash", "two"), (t1 - t0, t2 - t1, t3 - t2)):
            t[name].append(dt)
    med = {k: statistics.median(x) for k, x in t.items()}

    def leg(name):
        return {"tokens_per_s": n / med[name], "median_ms": med[name] * 1e3, "all_ms": [x * 1e3 for x in t[name]],
                "spread_ms": (max(t[name]) - min(t[name])) * 1e3}
    out = {
        "tokens": n, "passes": args.passes, "host_threads": threads,
        "payload_bytes": len(base64.urlsafe_b64decode(pool[0].split(b".")[1] + b"==")),
        "access_token_bytes": len(ats[0]),
        "match_blob_args_nonce": leg("nonce"), "match_blob_args_nonce_at_hash": dict(leg("hash"), **hstats),
        "nonce_then_verify_access_token_batch": leg("two"),
        "hash_over_workaround": med["two"] / med["hash"], "hash_over_nonce": med["nonce"] / med["hash"],
        # the acceptance condition: faster than the workaround by more than the spread of the laps
        "slowest_hash_ms": max(t["hash"]) * 1e3, "fastest_workaround_ms": min(t["two"]) * 1e3,
        "beats_workaround_beyond_spread": max(t["hash"]) < min(t["two"])}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
