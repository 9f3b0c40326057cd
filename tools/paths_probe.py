#!/usr/bin/env python3
"""Validator.SelectBlob by path against selecting the whole parent object and
against ValidateBlob, in one process.

tools/select_probe.py's pool and key set -- ES256 tokens signed for the 4 P-256
kids (tools/tokgen), served by a JWKS key set, "scope" and "roles" added to
every payload -- with one more member: "realm_access":{"roles":[...]}.  After
one warm pass of each entry three legs alternate for --passes timed passes each:

  path    SelectBlob(["scope", Path("realm_access", "roles")])
  parent  SelectBlob(["scope", "realm_access"]): the whole object, parsed from
          its span and marshalled again, for the caller to index
  full    ValidateBlob

The medians, the ratios and the CAPJWT_TRACE phase laps of one more pass of each
are printed as one JSON line.  The three accept arrays must be identical, the
scan must have decided every token (host == 0), and the path leg's columns are
checked against the payloads of a sample of the pool.

  python tools/paths_probe.py [--tokens 1048576] [--passes 5] [--kernels]

--kernels: instead of the three legs, three passes each of SelectBlobEach by
name (k_claims_select_each) and of the path leg (k_claims_paths_each) on the
same payloads, for a run under `rocprofv3 --kernel-trace --stats`: the two
kernels' times side by side in the kernel statistics.
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

EXTRA = '"roles":["admin","dev"],"scope":"read write","realm_access":{"roles":["offline_access","uma_authorization"]},'


def walk(claims, el):
    cur = claims
    for c in (el if isinstance(el, tuple) else (el,)):
        if not isinstance(cur, dict) or c not in cur:
            return False, None
        cur = cur[c]
    return True, cur


def check_columns(pool, names, cols):
    """the selected values of every 4099th token, from the columns, equal the payload's"""
    n = len(pool)
    for name, c in zip(names, cols["sel"]):
        off = struct.unpack("<%dI" % (n + 1), c["text_off"])
        for i in range(0, n, 4099):
            seg = pool[i].split(b".")[1]
            claims = json.loads(base64.urlsafe_b64decode(seg + b"=" * (-len(seg) % 4)))
            text = c["text"][off[i]:off[i + 1]]
            present, want = walk(claims, name)
            if isinstance(want, str):
                assert c["type"][i] == 1 and text.decode() == want, (i, name, text)
            elif isinstance(want, (list, dict)):
                assert c["type"][i] in (7, 8) and json.loads(text) == want, (i, name, text)
            else:
                assert (c["type"][i] == 0) == (not present) and text == b"", (i, name, text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1 << 20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    from cap_amd import jwt, _capjwt_host
    by_path = ["scope", jwt.Path("realm_access", "roles")]
    by_parent = ["scope", "realm_access"]
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
    v.ValidateBlob(b"\n".join(pool[:4096]), e)           # JWKS fetch + key staging
    ks.WaitTables()
    want = v.ValidateBlob(blob, e)                        # one warm pass of each
    pstats, ostats = {}, {}
    cols = v.SelectBlob(blob, by_parent, e, ostats)
    assert cols["ok"] == want, "SelectBlob by name and ValidateBlob verdicts differ"
    check_columns(pool, by_parent, cols)
    cols = v.SelectBlob(blob, by_path, e, pstats)
    assert cols["ok"] == want, "SelectBlob by path and ValidateBlob verdicts differ"
    assert sum(want) == len(pool), f"accepted {sum(want)} of {len(pool)}"
    assert pstats == ostats == {"scanned": len(pool), "host": 0}, (pstats, ostats)
    check_columns(pool, by_path, cols)
    del cols
    if args.kernels:
        which = array.array("I", bytes(4 * len(pool)))
        for _ in range(3):
            a = v.SelectBlobEach(blob, by_parent, [e], which, ostats)
            b = v.SelectBlob(blob, by_path, e, pstats)
            assert a["ok"] == want and b["ok"] == want and ostats["host"] == 0 and pstats["host"] == 0
            del a, b
        print(json.dumps({"tokens": len(pool), "kernels": ["k_claims_select_each", "k_claims_paths_each"], "passes": 3}))
        return
    t_val, t_par, t_path = [], [], []
    for _ in range(args.passes):
        t0 = time.perf_counter()
        a = v.ValidateBlob(blob, e)
        t1 = time.perf_counter()
        b = v.SelectBlob(blob, by_parent, e, ostats)
        t2 = time.perf_counter()
        c = v.SelectBlob(blob, by_path, e, pstats)
        t3 = time.perf_counter()
        assert a == want and b["ok"] == want and c["ok"] == want and ostats["host"] == 0 and pstats["host"] == 0
        del b, c
        t_val.append(t1 - t0)
        t_par.append(t2 - t1)
        t_path.append(t3 - t2)
    _, ph_val = bench.with_trace_phases(lambda: v.ValidateBlob(blob, e))
    _, ph_par = bench.with_trace_phases(lambda: v.SelectBlob(blob, by_parent, e))
    _, ph_path = bench.with_trace_phases(lambda: v.SelectBlob(blob, by_path, e))
    mv, mo, mp = statistics.median(t_val), statistics.median(t_par), statistics.median(t_path)

    def leg(m, ts, ph):
        return {"tokens_per_s": len(pool) / m, "median_ms": m * 1e3, "all_ms": [t * 1e3 for t in ts], "phases_ms": ph}
    print(json.dumps({
        "tokens": len(pool), "passes": args.passes, "host_threads": threads,
        "payload_bytes": len(base64.urlsafe_b64decode(pool[0].split(b".")[1] + b"==")),
        "validate_blob": leg(mv, t_val, ph_val), "select_parent_blob": leg(mo, t_par, ph_par),
        "select_path_blob": dict(leg(mp, t_path, ph_path), scanned=pstats["scanned"], host=pstats["host"]),
        "path_over_validate": mv / mp, "path_over_parent": mo / mp}))


if __name__ == "__main__":
    main()
