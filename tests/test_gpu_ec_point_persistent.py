"""The persistent k_ec_point (kernels/ecdsa_impl.hpp): for P-256, one-wave
blocks take 64-token groups from a per-launch counter, and launch_chain caps
the grid.

Every case runs in a fresh child process (the knobs are read once per
process) with
  CAPJWT_DEBUG_EC_POINT=1          launches of every size run k_ec_point
  CAPJWT_DEBUG_EC_POINT_BLOCKS=n   the persistent kernel's grid is n blocks
  CAPJWT_TABLE_BUDGET_GB=0         key tables at the narrowest tier (the crafted
                                   exceptional tokens of ec_edge.json are for it)
and sends batches of golden-fixture tokens through the C ABI as resident
batches (jg_batch_stage / jg_batch_run, the path of the benchmark), twice each:
the second run of the same staged batch shows that the scalar launch rewinds
the group counter (left where the first run put it, every block would find no
group and the run's exception count would stay 0).  Every verdict is compared
with the oracle's.

A batch cycles through valid tokens (one per kid), tampered signatures, a
token whose signature is not base64url (prep rejects it: status != OK), and the
P-256 (P-384) tokens of ec_edge.json, whose exceptional members are appended
to the exception list from inside the group loop.  Tokens are grouped by key
in whole waves, so every key's last wave carries padding lanes; the ES256
batches of 64, 65 and 192 tokens are 5 groups each, the 1000-token one 18.

The debug grid is taken as given, so caps 1, 2 and 5 give fewer blocks than
groups (each block loops), as many, and -- one token, one group, at caps 2 and
5 -- blocks that find no group and must exit without touching anything.

The ES384 batch goes through the same template with the loop compiled out
(P-384 and P-521 keep one block per group, ec_point_persistent): the forced
k_ec_point<P384> at a small size, the cap ignored.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# grid cap -> [(alg, tokens in the batch)]
CASES = {
    1: [("ES256", 1), ("ES256", 64), ("ES256", 65), ("ES256", 192)],
    2: [("ES256", 1), ("ES256", 64), ("ES256", 65), ("ES256", 192)],
    5: [("ES256", 1), ("ES256", 64), ("ES256", 65), ("ES256", 192)],
    3: [("ES256", 1000), ("ES384", 200)],
}
CURVE = {"ES256": "P-256", "ES384": "P-384"}
EC_CLASS = {"ES256": 4, "ES384": 5}          # jg_batch_exceptions index of the curve


def pool(alg):
    """[(token dict, key dict)] the batches cycle through, and every key used."""
    from oracle import jws
    from tests import gpu_helpers as H
    keys, toks = H.golden()
    edge = json.load(open(os.path.join(ROOT, "tests", "golden", "ec_edge.json")))
    crv = CURVE[alg]
    gkeys = [k for k in keys if k.get("crv") == crv]
    ekeys = [k for k in edge["keys"] if k.get("crv") == crv]
    kid_of = {k["kid"]: k for k in gkeys + ekeys}
    sel = []
    for k in gkeys:
        mine = [t for t in toks if t["key"] == k["kid"] and t["alg"] == alg]
        sel += [t for t in mine if t["name"].startswith("valid-")][:1]
        sel += [t for t in mine if t["name"].startswith("tamper-sig")][:1]
    assert any(t["name"].startswith("valid-") for t in sel) and any(t["name"].startswith("tamper-sig") for t in sel)
    # a signature segment that is not base64url: the oracle's parser refuses it, prep sets status != OK
    v = next(t for t in sel if t["name"].startswith("valid-"))
    head, sig = v["token"].rsplit(".", 1)
    bad = dict(v, name="bad-b64-" + v["name"], token=head + "." + sig[:5] + "*" + sig[6:])
    assert jws.parse_jws(bad["token"]) is None
    sel.append(bad)
    sel += [t for t in edge["tokens"] if t["key"] in kid_of and jws.parse_jws(t["token"]) is not None
            and jws.parse_jws(t["token"]).alg == alg]
    assert sum(1 for t in sel if t.get("exceptional")) >= 3
    return sel, gkeys + ekeys


def child(cap):
    """Runs in the child: every batch of CASES[cap], twice; prints one JSON line."""
    sys.path.insert(0, ROOT)
    from cap_amd import _lib
    from oracle import jws
    from tests import gpu_helpers as H
    res = []
    for alg, n in CASES[cap]:
        sel, keys = pool(alg)
        kid_index = {k["kid"]: i for i, k in enumerate(keys)}
        okeys = {k["kid"]: jws.Key.from_fixture(k) for k in keys}
        want_of = {}
        for t in sel:
            p = jws.parse_jws(t["token"])
            want_of[t["name"]] = int(jws.verify_sig(p, okeys[t["key"]])) if p is not None else 0
        batch = [sel[i % len(sel)] for i in range(n)]
        ctx = _lib.Context()
        ctx.load_keys([H.abi_key(k) for k in keys])
        arena = _lib.Arena()
        for t in batch:
            # the job of a token the parser refuses is packed all the same, so it reaches prep
            head, sig = t["token"].rsplit(".", 1)
            arena.add(head.encode(), sig.encode(), alg, kid_index[t["key"]])
        want = [want_of[t["name"]] for t in batch]
        exc = sum(1 for t in batch if t.get("exceptional"))
        b = ctx.stage(arena)
        for run in range(2):
            out = list(b.run(want_verdicts=True))
            bad = [(i, batch[i]["name"], out[i], want[i]) for i in range(n) if out[i] != want[i]]
            res.append({"alg": alg, "n": n, "run": run, "bad": bad[:8], "accepted": sum(out),
                        "exceptions": b.exceptions()[EC_CLASS[alg]], "want_exceptions": exc,
                        "widths": sorted(set(ctx.table_widths()))})
        b.free()
        ctx.close()
    print("RESULT " + json.dumps(res))


@pytest.mark.gpu
@pytest.mark.parametrize("cap", sorted(CASES))
def test_persistent_point_kernel_under_grid_cap(cap):
    env = dict(os.environ, CAPJWT_DEBUG_EC_POINT="1", CAPJWT_DEBUG_EC_POINT_BLOCKS=str(cap),
               CAPJWT_TABLE_BUDGET_GB="0")
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--child", str(cap)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=110)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, f"cap {cap}: child failed\n{tail}"
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    res = json.loads(line[len("RESULT "):])
    assert [(x["alg"], x["n"]) for x in res] == [c for c in CASES[cap] for _ in range(2)]
    for x in res:
        what = f"cap {cap} {x['alg']} n={x['n']} run {x['run']}"
        assert x["bad"] == [], what
        assert x["exceptions"] == x["want_exceptions"], what       # the list is appended to once per run
        assert 0 < x["accepted"] < x["n"] or x["n"] == 1, what
        # narrowest tier of the curve's key tables (kernels/ecdsa.hpp)
        assert x["widths"] == [{"ES256": 20, "ES384": 16}[x["alg"]]], what


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    child(int(sys.argv[2]))
