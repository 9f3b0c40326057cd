"""ES256 through k_ec_point on the XYZZ accumulator (kernels/ecdsa_impl.hpp
ec_point_token, ec_point_xyzz), through the library (GPU).

Each case is a fresh child process (the knobs are read once per process) with
  CAPJWT_DEBUG_EC_POINT=1          launches of every size run k_ec_point
  CAPJWT_DEBUG_EC_POINT_BLOCKS=g   its grid is g one-wave blocks (1 and 3)
and the key tables at width 26 (the benchmark's) or 20 (the narrowest),
through jg_set_table_budget.  It stages ES256 batches of 1, 63, 64, 65 and
1000 tokens as resident batches and runs each twice.  A batch cycles through a
valid and a tampered token of a golden key and the P-256 tokens of
tests/golden/ec_edge.json: the exceptional pairs (the kernel must find
ZZ == 0 and hand the token to k_ec_exact) and x(R) = r + n (the accept test
on ZZ).  Every verdict must equal the oracle's and jg_batch_exceptions the
number of exceptional tokens in the batch.

Which edge tokens are exceptional depends on the key width.  The fixture file
states it for width 20; exceptional_at() recomputes it for any width from the
token's scalars in Python integers (the comb sum in the kernel's order by the
chord rule), must agree with the file at 20, and gives the count at 26."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [1, 63, 64, 65, 1000]
CASES = [(wq, grid) for wq in (26, 20) for grid in (1, 3)]
CLS_P256 = 4                                 # jg_batch_exceptions index of the curve


def edge():
    e = json.load(open(os.path.join(ROOT, "tests", "golden", "ec_edge.json")))
    keys = [k for k in e["keys"] if k.get("crv") == "P-256"]
    kids = {k["kid"] for k in keys}
    return keys, [t for t in e["tokens"] if t["key"] in kids and t["alg"] == "ES256"]


def exceptional_at(tok, key, wq):
    """whether the comb sum of the token's u1 G + u2 Q, added in k_ec_point's
    order (window w of G, then window w of Q), meets P == +-Q"""
    import hashlib
    from oracle import jws
    from tests import scalar_model as M
    from tests import table_model as T
    from tests import xyzz_model as X
    cls = T.CLS_P256
    p = jws.parse_jws(tok["token"])
    sig = p.signature
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    sc = M.ec_scalars(cls, M.ES256, r, s, hashlib.sha256(p.signing_input).digest())
    if sc is None:
        return False
    G, Q = T.ec_generator(cls), (int(key["x"], 16), int(key["y"], 16))
    wg = M.EC_WG[cls]
    d1, c1 = M.recode(sc[0], wg, M.ec_windows(cls, wg), True)
    d2, c2 = M.recode(sc[1], wq, M.ec_windows(cls, wq), True)
    assert c1 == 0 and c2 == 0
    pts, sg = [], []
    for w in range(max(len(d1), len(d2))):
        for d, width, base in ((d1, wg, G), (d2, wq, Q)):
            if w < len(d) and d[w] != 0:
                pts.append(T.ec_mul(cls, abs(d[w]) << (width * w), base))
                sg.append(1 if d[w] > 0 else -1)
    return X.reference(pts, sg)[1]


def pool():
    """[token dict] a batch cycles through, every key used, and the oracle's verdict per token name"""
    from oracle import jws
    from tests import gpu_helpers as H
    gkeys, toks = H.golden()
    gkey = next(k for k in gkeys if k["kid"] == "p256-a")
    mine = [t for t in toks if t["key"] == "p256-a" and t["alg"] == "ES256"]
    sel = [next(t for t in mine if t["name"].startswith("valid-")),
           next(t for t in mine if t["name"].startswith("tamper-sig"))]
    ekeys, etoks = edge()
    sel += etoks
    keys = [gkey] + ekeys
    okeys = {k["kid"]: jws.Key.from_fixture(k) for k in keys}
    want = {t["name"]: int(jws.verify_sig(jws.parse_jws(t["token"]), okeys[t["key"]])) for t in sel}
    for t in etoks:
        assert want[t["name"]] == t["verdict"], t["name"]
    return sel, keys, want


def child(wq, exc_names):
    """Runs in the child: every size, twice; prints one JSON line."""
    sys.path.insert(0, ROOT)
    import bench
    from cap_amd import _lib
    from tests import gpu_helpers as H
    sel, keys, want_of = pool()
    kid_index = {k["kid"]: i for i, k in enumerate(keys)}
    ctx = _lib.Context()
    ctx.set_table_budget(len(keys) * bench.table_bytes("p256", wq))
    ctx.load_keys([H.abi_key(k) for k in keys])
    widths = sorted(set(ctx.table_widths()))
    res = []
    for n in SIZES:
        batch = [sel[i % len(sel)] for i in range(n)]
        arena = _lib.Arena()
        for t in batch:
            head, sig = t["token"].rsplit(".", 1)
            arena.add(head.encode(), sig.encode(), "ES256", kid_index[t["key"]])
        want = [want_of[t["name"]] for t in batch]
        b = ctx.stage(arena)
        for run in range(2):
            out = list(b.run(want_verdicts=True))
            bad = [(i, batch[i]["name"], out[i], want[i]) for i in range(n) if out[i] != want[i]]
            res.append({"n": n, "run": run, "bad": bad[:8], "accepted": sum(out), "want_accepted": sum(want),
                        "exceptions": b.exceptions()[CLS_P256],
                        "want_exceptions": sum(1 for t in batch if t["name"] in exc_names), "widths": widths})
        b.free()
    ctx.close()
    print("RESULT " + json.dumps(res))


@pytest.fixture(scope="module")
def exceptional_names():
    """width -> names of the edge tokens whose comb sum is exceptional at that key width"""
    ekeys, etoks = edge()
    kof = {k["kid"]: k for k in ekeys}
    out = {wq: {t["name"] for t in etoks if exceptional_at(t, kof[t["key"]], wq)} for wq in (26, 20)}
    stated = {t["name"] for t in etoks if t.get("exceptional")}
    assert out[20] == stated and len(stated) >= 3          # the fixture file's own statement, at the width it is for
    assert len(out[26]) >= 2                                # Q = +-G with u1 = u2 = 1: exceptional at any width
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("wq,grid", CASES)
def test_es256_batches_through_the_forced_point_kernel(wq, grid, exceptional_names):
    env = dict(os.environ, CAPJWT_DEBUG_EC_POINT="1", CAPJWT_DEBUG_EC_POINT_BLOCKS=str(grid))
    env.pop("CAPJWT_TABLE_BUDGET_GB", None)
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--child", str(wq),
                        json.dumps(sorted(exceptional_names[wq]))], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=170)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, f"W = {wq}, grid {grid}: child failed\n{tail}"
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    res = json.loads(line[len("RESULT "):])
    assert [(x["n"], x["run"]) for x in res] == [(n, run) for n in SIZES for run in range(2)]
    for x in res:
        what = f"W = {wq}, grid {grid}, n = {x['n']}, run {x['run']}"
        assert x["widths"] == [wq], what
        assert x["bad"] == [], what
        assert x["accepted"] == x["want_accepted"], what
        assert x["exceptions"] == x["want_exceptions"], what     # appended once per run, the counter rewound
        if x["n"] >= 63:
            assert 0 < x["accepted"] < x["n"] and x["want_exceptions"] >= 2, what


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child(int(sys.argv[2]), set(json.loads(sys.argv[3])))
