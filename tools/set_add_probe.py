#!/usr/bin/env python3
"""Adding to a resident set on the device (jg_set_add, ClaimSet.Add) against the
workaround it replaces, the whole set loaded again (jg_set_load,
ClaimSet.Replace), in one process.

The set holds --members members (2^20), half of them jtis of tools/match_probe.py's
pool (the even token indices), half strings that occur in no token.  Each lap
adds --add (1,024) members that are not in it: odd token indices, so the masks of
the last pass show them.  Legs, alternating, --passes (5) laps each, every lap
printed:

  abi_add      jg_set_add of the lap's members; the table has room (it doubled once)
  abi_reload   jg_set_load of all members so far plus the lap's, under another id
  abi_double   jg_set_add of the lap's members to a set just loaded with 2^20
               members, whose table is exactly full: one rehash into twice the slots
  py_add       ClaimSet.Add of the lap's members
  py_replace   ClaimSet.Replace with all members so far plus the lap's

The ABI legs time the C call alone (the arguments are packed before).  After the
legs one MatchBlobArgs([InSet("jti", set)]) pass over the pool must give the
masks of the Python evaluation.  The acceptance condition is checked and the run
fails without it: at both layers the slowest add lap is under the fastest reload
lap.  One JSON line; --out writes it to a file as well.

  python tools/set_add_probe.py [--tokens 1048576] [--members 1048576] [--add 1024] [--passes 5] [--kernels]

--kernels: instead of the legs, three MatchBlobArgs passes against a set that was
added to (loaded with half the members, the other half added in 64 calls) and
three against a set loaded whole with the same members, alternating, for a run
under `rocprofv3 --kernel-trace --stats`; prints both sets' maxprobe and slots.
"""
import argparse
import ctypes
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


def packed(members):
    """(blob, spans array, count) as jg_set_load / jg_set_add take them"""
    from cap_amd import _lib
    blob = b"".join(members)
    sp = (_lib.JgSArg * max(1, len(members)))()
    o = 0
    for x, m in zip(sp, members):
        x.off, x.len = o, len(m)
        o += len(m)
    return blob, sp, len(members)


def timed_ms(f):
    t0 = time.perf_counter()
    rc = f()
    return (time.perf_counter() - t0) * 1e3, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 20)
    ap.add_argument("--members", type=int, default=1 << 20)
    ap.add_argument("--add", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    from cap_amd import jwt, _capjwt_host, _lib
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
    half = args.members // 2
    base = ["%d" % (2 * k) for k in range(half)] + ["revoked-%d" % k for k in range(args.members - half)]
    lap_members = lambda leg, lap: ["%d" % (2 * ((leg * args.passes + lap) * args.add + j) + 1) for j in range(args.add)]

    def evaluate(members):
        s = set(members)
        return [int(("%d" % i) in s) for i in range(n)]

    def masks_of(cset):
        stats = {}
        cols = v.MatchBlobArgs(blob, [jwt.InSet("jti", cset)], [], [], e, stats)
        assert stats == {"scanned": n, "host": 0} and sum(cols["ok"]) == n, stats
        return list(struct.unpack("<%dI" % n, cols["match"]))

    if args.kernels:
        step = (args.members - half) // 64
        grown = v.NewClaimSet(base[:half], seed=1)
        for k in range(64):
            grown.Add(base[half + k * step:half + (k + 1) * step if k < 63 else args.members])
        whole = v.NewClaimSet(base, seed=1)
        assert grown.info()["n"] == whole.info()["n"] == args.members
        want = evaluate(base)
        for _ in range(3):
            assert masks_of(grown) == want and masks_of(whole) == want
        print(json.dumps({"tokens": n, "passes": 3, "order": ["added-to set", "set loaded whole"], "added_to": grown.info(),
                          "loaded_whole": whole.info()}))
        return

    L = _lib.lib()
    ctx = _lib.Context()
    t = {k: [] for k in ("abi_add", "abi_reload", "abi_double", "py_add", "py_replace")}
    bb, bs, bn = packed([m.encode() for m in base])
    assert L.jg_set_load(ctx.h, 0, bb, len(bb), ctypes.cast(bs, ctypes.c_void_p), bn, 7) == 0, ctx.error()
    have = list(base)
    # the table of exactly 2 n slots doubles at the first add: done here, outside abi_add's laps
    first = ["first-%d" % k for k in range(args.add)]
    fb, fs, fn = packed([m.encode() for m in first])
    assert L.jg_set_add(ctx.h, 0, fb, len(fb), ctypes.cast(fs, ctypes.c_void_p), fn, None) == 0, ctx.error()
    have += first
    cset = v.NewClaimSet(base, seed=7)
    cset.Add(first)
    infos = {}
    for lap in range(args.passes):
        new = lap_members(0, lap)
        nb, ns, nn = packed([m.encode() for m in new])
        added = ctypes.c_uint32(0)
        ms, rc = timed_ms(lambda: L.jg_set_add(ctx.h, 0, nb, len(nb), ctypes.cast(ns, ctypes.c_void_p), nn, ctypes.byref(added)))
        assert rc == 0 and added.value == args.add, (rc, added.value, ctx.error())
        t["abi_add"].append(ms)
        have += new
        ab, as_, an = packed([m.encode() for m in have])
        ms, rc = timed_ms(lambda: L.jg_set_load(ctx.h, 1, ab, len(ab), ctypes.cast(as_, ctypes.c_void_p), an, 7))
        assert rc == 0, ctx.error()
        t["abi_reload"].append(ms)
        assert ctx.set_info(0)["n"] == ctx.set_info(1)["n"] == len(have)
        assert L.jg_set_load(ctx.h, 2, bb, len(bb), ctypes.cast(bs, ctypes.c_void_p), bn, 7) == 0, ctx.error()
        before = ctx.set_info(2)
        ms, rc = timed_ms(lambda: L.jg_set_add(ctx.h, 2, nb, len(nb), ctypes.cast(ns, ctypes.c_void_p), nn, None))
        assert rc == 0 and ctx.set_info(2)["nslots"] == 2 * before["nslots"], ctx.error()
        t["abi_double"].append(ms)
        ms, cnt = timed_ms(lambda: cset.Add(new))
        assert cnt == args.add
        t["py_add"].append(ms)
        ms, _ = timed_ms(lambda: cset.Replace(have, seed=7))
        t["py_replace"].append(ms)
        infos = {"added_to": ctx.set_info(0), "reloaded": ctx.set_info(1), "doubled": ctx.set_info(2)}
        print("lap %d: " % lap + ", ".join("%s %.2f ms" % (k, x[-1]) for k, x in t.items()), file=sys.stderr, flush=True)
    # the set that was added to, on the scan: Add once more so that the last thing done to it is an add
    last = lap_members(1, 0)
    assert cset.Add(last) == args.add
    have += last
    assert masks_of(cset) == evaluate(have), "the masks differ from the Python evaluation"
    ctx.close()
    leg = lambda name: {"median_ms": statistics.median(t[name]), "all_ms": t[name]}
    out = {"tokens": n, "members": args.members, "add": args.add, "passes": args.passes, "host_threads": threads,
           **{k: leg(k) for k in t}, "set_info": infos, "claim_set_info": cset.info(),
           "abi_slowest_add_ms": max(t["abi_add"]), "abi_fastest_reload_ms": min(t["abi_reload"]),
           "py_slowest_add_ms": max(t["py_add"]), "py_fastest_replace_ms": min(t["py_replace"]),
           "abi_double_slowest_ms": max(t["abi_double"]),
           "add_beats_reload_beyond_spread": max(t["abi_add"]) < min(t["abi_reload"]) and max(t["py_add"]) < min(t["py_replace"])}
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not out["add_beats_reload_beyond_spread"]:
        raise SystemExit("acceptance: an add's slowest lap is not under the whole reload's fastest lap")


if __name__ == "__main__":
    main()
