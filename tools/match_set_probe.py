#!/usr/bin/env python3
"""Validator.MatchBlobArgs with InSet on a resident set -- is jti revoked? --
against MatchBlob with one constant predicate, CheckBlob, and the workaround it
replaces (RegisteredBlob and a Python `set` lookup over its jti column), in one
process.

tools/match_probe.py's pool and key set: 1,048,576 ES256 tokens signed for the 4
P-256 kids (tools/tokgen), served by a JWKS key set; jti is the decimal token
index.  The set holds --members members (2^20): half of them jtis of the pool
(the even indices), half strings that occur in no token.  After one warm pass of
each entry four legs alternate for --passes timed passes each:

  inset   MatchBlobArgs([InSet("jti", revoked)]): a mask per token comes back
  match   MatchBlob([Equals("jti", one value)]): one constant predicate
  check   CheckBlob: the verdict alone
  python  the workaround: RegisteredBlob, then `in` on a Python set per token
          over its jti column

The accept arrays must be identical, the scan must have decided every token
(host == 0) and the masks must equal the workaround's answers.  The acceptance
condition is checked and the run fails without it: the new call's slowest lap is
under the workaround's fastest lap.  Also printed: NewClaimSet of the set in ms
(CAPJWT_LOAD_TRACE=1 makes the library print its host build and its upload apart
on stderr).  One JSON line; --out writes it to a file as well.

  python tools/match_set_probe.py [--tokens 1048576] [--members 1048576] [--passes 5] [--kernels]

--kernels: instead of the legs, three passes each of the inset leg against the
big set (k_claims_match_set), against a set of 2^10 members, and of
MatchBlobArgs([Equals("jti", one value)]) -- the Equals leg without an operand,
which launches k_claims_match_args -- on the same payloads, for a run under
`rocprofv3 --kernel-trace --stats` (no counters, no other tracing).
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the pool)

T0 = 1611699344


def members_of(count, n):
    half = count // 2
    return ["%d" % (2 * k) for k in range(half)] + ["revoked-%d" % k for k in range(count - half)], \
        [int(i % 2 == 0 and i < 2 * half) for i in range(n)]


def workaround(v, blob, e, revoked, n, stats=None):
    """RegisteredBlob and the lookup in Python -> (ok, masks)"""
    cols = v.RegisteredBlob(blob, e, stats)
    offs, data = cols["jti"]
    off = struct.unpack("<%dI" % (n + 1), offs)
    return cols["ok"], [int(data[off[i]:off[i + 1]] in revoked) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 20)
    ap.add_argument("--members", type=int, default=1 << 20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    from cap_amd import jwt, _capjwt_host
    threads = _capjwt_host.host_threads()
    kids = bench.E2E_KIDS
    pool = bench.gen_tokens("ES256", args.tokens, bench.golden_keypaths(kids), threads, "setprobe")
    n = len(pool)
    jwk = [{"kty": "EC", "kid": f"kid-{i:02d}", "crv": "P-256", **xy} for i, xy in enumerate(bench.p256_jwk_xy(kids))]
    jwks = json.dumps({"keys": jwk}).encode()
    ks, err = jwt.NewJSONWebKeySet(None, "https://bench.example/jwks", "",
                                   lambda url, ca: {"status": 200, "body": jwks, "max_age": 3600})
    assert err is None, err
    v, _ = jwt.NewValidator(ks)
    e = jwt.Expected(Issuer="https://example.com/", Audiences=["www.example.com"], SigningAlgorithms=["ES256"],
                     Now=lambda: T0 + 60)
    blob = b"\n".join(pool)
    v.CheckBlob(b"\n".join(pool[:4096]), e)               # JWKS fetch + key staging
    ks.WaitTables()
    members, want_masks = members_of(args.members, n)
    t0 = time.perf_counter()
    revoked = v.NewClaimSet(members)
    load_ms = (time.perf_counter() - t0) * 1e3
    info = revoked.info()
    assert not info["host_only"] and info["n"] == args.members, info
    pyset = set(m.encode() for m in members)              # the workaround's own copy, built outside the timed legs
    requires = [jwt.InSet("jti", revoked)]
    constant = [jwt.Equals("jti", "%d" % (n // 2))]
    cstats, pstats, mstats, sstats = {}, {}, {}, {}
    want = v.CheckBlob(blob, e, cstats)                   # one warm pass of each
    ok, pmasks = workaround(v, blob, e, pyset, n, pstats)
    assert ok == want, "RegisteredBlob and CheckBlob verdicts differ"
    cols = v.MatchBlob(blob, constant, e, mstats)
    assert cols["ok"] == want and sum(struct.unpack("<%dI" % n, cols["match"])) == 1, "MatchBlob"
    cols = v.MatchBlobArgs(blob, requires, [], [], e, sstats)
    assert cols["ok"] == want, "MatchBlobArgs and CheckBlob verdicts differ"
    assert sum(want) == n, f"accepted {sum(want)} of {n}"
    assert cstats == pstats == mstats == sstats == {"scanned": n, "host": 0}, (cstats, pstats, mstats, sstats)
    masks = list(struct.unpack("<%dI" % n, cols["match"]))
    assert masks == pmasks == want_masks, "the masks differ from the workaround's or from the pool's"
    del cols
    if args.kernels:
        small = v.NewClaimSet(members_of(1 << 10, n)[0])
        for _ in range(3):
            a = v.MatchBlobArgs(blob, requires, [], [], e, sstats)
            b = v.MatchBlobArgs(blob, [jwt.InSet("jti", small)], [], [], e, sstats)
            c = v.MatchBlobArgs(blob, constant, [], [], e, mstats)
            assert a["ok"] == want and b["ok"] == want and c["ok"] == want and sstats["host"] == 0 and mstats["host"] == 0
            del a, b, c
        print(json.dumps({"tokens": n, "passes": 3, "order": ["inset 2^20: k_claims_match_set", "inset 2^10: k_claims_match_set",
                                                             "equals: k_claims_match_args"]}))
        return
    t = {"inset": [], "match": [], "check": [], "python": []}
    for _ in range(args.passes):
        t0 = time.perf_counter()
        a = v.MatchBlobArgs(blob, requires, [], [], e, sstats)
        t1 = time.perf_counter()
        b = v.MatchBlob(blob, constant, e, mstats)
        t2 = time.perf_counter()
        c = v.CheckBlob(blob, e, cstats)
        t3 = time.perf_counter()
        d, dm = workaround(v, blob, e, pyset, n, pstats)
        t4 = time.perf_counter()
        assert a["ok"] == want and b["ok"] == want and c == want and d == want
        assert sstats["host"] == 0 and mstats["host"] == 0 and cstats["host"] == 0 and pstats["host"] == 0
        assert a["match"] == struct.pack("<%dI" % n, *dm)
        del a, b, c, d, dm
        for name, dt in zip(("inset", "match", "check", "python"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            t[name].append(dt)
    med = {k: statistics.median(x) for k, x in t.items()}
    leg = lambda name: {"tokens_per_s": n / med[name], "median_ms": med[name] * 1e3, "all_ms": [x * 1e3 for x in t[name]]}
    out = {"tokens": n, "members": args.members, "passes": args.passes, "host_threads": threads, "set_info": info,
           "new_claim_set_ms": load_ms, "match_blob_args_inset": leg("inset"), "match_blob_equals": leg("match"),
           "check_blob": leg("check"), "registered_blob_plus_python_set": leg("python"),
           "inset_over_workaround": med["python"] / med["inset"], "inset_over_match": med["match"] / med["inset"],
           "slowest_inset_ms": max(t["inset"]) * 1e3, "fastest_workaround_ms": min(t["python"]) * 1e3,
           "beats_workaround_beyond_spread": max(t["inset"]) < min(t["python"])}
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not out["beats_workaround_beyond_spread"]:
        raise SystemExit("acceptance: the new call's slowest lap is not under the workaround's fastest lap")


if __name__ == "__main__":
    main()
