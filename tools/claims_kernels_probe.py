#!/usr/bin/env python3
"""All seven claims kernels on the same 524,288 payload segments (payloads of about
205 bytes, 64 profiles, two names, three paths), PASSES launches each, through the
_lib.Context entries of this tree.

  rocprofv3 --kernel-trace --stats -d OUT -o kt --output-format csv -- python tools/claims_kernels_probe.py

The kernel statistics of such a run (of its own, no counters) hold the seven
kernels' times side by side.  The program prints one JSON line with the SHA-256
of every entry's outputs and its codes, so two builds can be compared: the same
line means the same bytes from all seven kernels."""
import base64
import collections
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cap_amd import _lib  # noqa: E402

N = 1 << 19
PASSES = 4
T0 = 1700000000


def seg(k):
    p = (b'{"iss":"https://example.com/","aud":["www.example.com","api-%d"],"sub":"user-%d","exp":%d,"iat":%d,'
         b'"scope":"read write","realm_access":{"roles":["admin","dev"]},"cnf":{"jkt":"thumb-%d"}}'
         % (k % 7, k, T0 + 600 + k % 50, T0 - 60, k))
    return base64.urlsafe_b64encode(p).rstrip(b"=")


def main():
    pool = [seg(k) for k in range(4096)]
    arena = bytearray()
    spans = []
    for i in range(N):
        s = pool[i % len(pool)]
        spans.append((len(arena), len(s)))
        arena += s
    arena = bytes(arena)

    def ex(k):
        return {"issuer": b"https://example.com/", "audiences": [b"api-%d" % k, b"www.example.com"], "now_sec": T0 + k,
                "now_nsec": 0, "skew_ns": 0, "exp_leeway_s": 0, "nbf_leeway_s": 0}
    sets = [ex(k) for k in range(64)]
    jobs = [(o, ln, i % 64) for i, (o, ln) in enumerate(spans)]
    names = [b"scope", b"realm_access"]
    paths = [[b"scope"], [b"realm_access", b"roles"], [b"cnf", b"jkt"]]
    ctx = _lib.Context([0])
    legs = {
        "k_claims_scan": lambda: ctx.claims_scan(arena, spans, sets[0]),
        "k_claims_extract": lambda: ctx.claims_extract(arena, spans, sets[0]),
        "k_claims_select": lambda: ctx.claims_select(arena, spans, sets[0], names),
        "k_claims_scan_each": lambda: ctx.claims_each(arena, jobs, sets),
        "k_claims_extract_each": lambda: ctx.claims_each(arena, jobs, sets, mode="extract"),
        "k_claims_select_each": lambda: ctx.claims_each(arena, jobs, sets, mode="select", names=names),
        "k_claims_paths_each": lambda: ctx.claims_paths(arena, jobs, sets, paths),
    }
    res = {}
    for p in range(PASSES):
        for name, leg in legs.items():
            out = leg()
            out = (out,) if isinstance(out, bytes) else tuple(bytes(x) for x in out)
            h = hashlib.sha256(b"".join(out)).hexdigest()
            assert res.setdefault(name, {"sha256": h, "codes": dict(collections.Counter(out[0]))})["sha256"] == h, name
    ctx.close()
    print(json.dumps({"jobs": N, "passes": PASSES, "legs": res}))


if __name__ == "__main__":
    main()
