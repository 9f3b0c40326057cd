#!/usr/bin/env python3
"""What a set-membership predicate costs in the claims scan, through the C ABI.

1,048,576 payload segments whose `jti` is the decimal token index, and a
resident set of 2^20 members (--members): half of them jtis of the pool (the
even indices), half strings that occur in no token.  The legs alternate in one
process, medians of --laps:

  in_set     jg_claims_match_set, IN_SET(jti, the set)
  in_set_1k  the same against a set of 2^10 members
  equals     jg_claims_match, EQUALS(jti, one value)
  equals_args  jg_claims_match_args, the same EQUALS and no column: k_claims_match_args,
             the kernel the set kernel grew out of, on the same payloads
  scan       jg_claims_each, the verdict alone

Every leg times the C call alone (upload, kernel, copy back); the arguments are
built once.  The masks must be "the index is even" for every token and the scan
must decide every token.  Also printed: jg_set_load of the big set in ms (with
CAPJWT_LOAD_TRACE=1 the library prints its host build and its upload apart, on
stderr).  The
entries above the C ABI (Validator, jwt) do not take set predicates yet, so the
RegisteredBlob + Python-set workaround is not a leg here.  Prints one JSON
object; --out writes it to a file as well.

Kernel times: run this file under `rocprofv3 --kernel-trace --stats` (no
counters, no other tracing) with --laps 3 and read k_claims_match_set against
k_claims_match_args and k_claims_match_each in its statistics.
"""
import argparse
import base64
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cap_amd import _lib  # noqa: E402

T0 = 1611699344


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 20)
    ap.add_argument("--members", type=int, default=1 << 20)
    ap.add_argument("--laps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    n = a.tokens
    head = b'{"iss":"https://example.com/","sub":"alice@example.com","aud":"www.example.com","exp":%d,"iat":%d,"jti":"' % (T0 + 600, T0)
    segs = [base64.urlsafe_b64encode(head + b"%d" % i + b'"}').rstrip(b"=") for i in range(n)]
    arena = b"".join(segs)
    cj = (_lib.JgCJob * n)()
    o = 0
    for j, s in zip(cj, segs):
        j.off, j.len, j.flags = o, len(s), 0
        o += len(s)
    ctx = _lib.Context()
    L = _lib.lib()
    half = a.members // 2
    big = [b"%d" % (2 * k) for k in range(half)] + [b"revoked-%d" % k for k in range(a.members - half)]
    t = time.perf_counter()
    ctx.set_load(0, big, 0x5eed)
    load_ms = (time.perf_counter() - t) * 1e3                 # with the Python side's join of the members
    small = [b"%d" % (2 * k) for k in range(512)] + [b"revoked-%d" % k for k in range(512)]
    ctx.set_load(1, small, 0x5eed)
    e, _keep = _lib._jg_expect({"issuer": b"https://example.com/", "audiences": [b"www.example.com"], "now_sec": T0 + 30,
                                "now_nsec": 0, "skew_ns": 0, "exp_leeway_s": 0, "nbf_leeway_s": 0})
    ps, _k1 = _lib._jg_paths([[b"jti"]])
    q_set, _k2 = _lib._jg_preds([(0, _lib.PRED_IN_SET, b"\0")])
    q_eq, _k3 = _lib._jg_preds([(0, _lib.PRED_EQUALS, b"524288")])
    s_big, s_small = _lib._jg_setargs([0]), _lib._jg_setargs([1])
    no_args = _lib.JgArgs()                                   # no column of either kind
    codes = ctypes.create_string_buffer(n)
    masks = (ctypes.c_uint32 * n)()
    mp = ctypes.cast(masks, ctypes.c_void_p)

    def call(rc):
        if rc != 0:
            raise SystemExit("rc=%d: %s" % (rc, ctx.error()))

    legs = {
        "in_set": lambda: call(L.jg_claims_match_set(ctx.h, arena, len(arena), cj, n, ctypes.byref(e), 1, ctypes.byref(ps),
                                                     ctypes.byref(q_set), None, None, ctypes.byref(s_big), codes, mp)),
        "in_set_1k": lambda: call(L.jg_claims_match_set(ctx.h, arena, len(arena), cj, n, ctypes.byref(e), 1, ctypes.byref(ps),
                                                        ctypes.byref(q_set), None, None, ctypes.byref(s_small), codes, mp)),
        "equals": lambda: call(L.jg_claims_match(ctx.h, arena, len(arena), cj, n, ctypes.byref(e), 1, ctypes.byref(ps),
                                                 ctypes.byref(q_eq), codes, mp)),
        "equals_args": lambda: call(L.jg_claims_match_args(ctx.h, arena, len(arena), cj, n, ctypes.byref(e), 1, ctypes.byref(ps),
                                                           ctypes.byref(q_eq), ctypes.byref(no_args), codes, mp)),
        "scan": lambda: call(L.jg_claims_each(ctx.h, arena, len(arena), cj, n, ctypes.byref(e), 1, None, codes, None, None)),
    }
    # correctness first (this is also the warm-up of every leg)
    legs["in_set"]()
    host = sum(1 for c in codes.raw if c == _lib.CL_HOST)
    wrong = sum(1 for i in range(n) if masks[i] != (1 if i % 2 == 0 and i < 2 * half else 0))
    legs["in_set_1k"]()
    wrong_1k = sum(1 for i in range(n) if masks[i] != (1 if i % 2 == 0 and i < 1024 else 0))
    legs["equals"]()
    wrong_eq = sum(1 for i in range(n) if masks[i] != (1 if i == 524288 else 0))
    legs["equals_args"]()
    wrong_eq += sum(1 for i in range(n) if masks[i] != (1 if i == 524288 else 0))
    legs["scan"]()
    laps = {k: [] for k in legs}
    for _ in range(a.laps):
        for k, f in legs.items():
            t = time.perf_counter()
            f()
            laps[k].append(round((time.perf_counter() - t) * 1e3, 2))
    out = {"tokens": n, "members": a.members, "arena_bytes": len(arena), "set_info": ctx.set_info(0), "set_load_ms": round(load_ms, 1),
           "host_tokens": host, "wrong_masks": {"in_set": wrong, "in_set_1k": wrong_1k, "equals": wrong_eq},
           "legs": {k: {"median_ms": statistics.median(v), "laps_ms": v} for k, v in laps.items()}}
    ctx.close()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if host or wrong or wrong_1k or wrong_eq:
        raise SystemExit("the masks are not the answers")


if __name__ == "__main__":
    main()
