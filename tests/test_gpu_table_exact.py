"""Comb tables as built in HBM against big-integer arithmetic (GPU).

Every ECDSA / EdDSA verdict is a sum of comb-table entries; the tables are
built on the device (k_ec_table_base_g / k_ec_table_g / k_ec_table_base_keys /
k_ec_table_keys, k_ed_table_base_b / k_ed_table_b / k_ed_table_base_keys /
k_ed_table_keys) from what k_ec_keyprep / k_ed_decode leave in the key blob.
jg_debug_table_read copies raw entries back; tests/table_model.py decodes them
(asserting canonical form) and gives d * 2^(W w) * P for entry (w, d).  Per
table the sample set of table_model.sample_entries is read: d in {1, 2, 3,
NE - 1, NE} of every window, the first and last entry, the entries around
every multiple of the 2^23-entry build slice (kernels/tables.hpp), and 64
seeded random (w, d).  Every comparison is integer equality; the stride's
padding words are not looked at.

  * the generator / base-point tables of all four curves;
  * a key table at every width tier, widened by the background upgrader (its
    builds are sliced) except the narrowest, which jg_keys_load builds; entry
    (0, 1) is Q in Montgomery form / -A, so k_ec_keyprep and k_ed_decode are
    pinned exactly;
  * the same keys built unsliced by a child process under CAPJWT_TABLES_SYNC=1:
    the samples again, and its jg_debug_table_digest of every table equals
    the upgrader-built table's, which extends exactness from the samples to
    every word of those tables;
  * three keys in one load with an invalid one in the middle: the invalid key
    reports width 0 and has no table to read, and both neighbours' tables,
    built by one launch over the load's valid keys (blockIdx.y -> idx[k]),
    are exact;
  * Ed25519 keys of small order, with x = 0 and the sign bit set, and with a
    non-canonical y.  By Go's Point.SetBytes rule (table_model docstring) all
    of them are valid keys, so each has a table, exact like any other: the
    complete addition holds on small-order points;
  * the hook's refusals copy nothing.

Each case prints its load and check wall times (pytest -s)."""
import json
import os
import subprocess
import sys
import time

import pytest

from tests import scalar_model as M
from tests import table_model as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAB = {"P-256": "p256", "P-384": "p384", "P-521": "p521", "Ed25519": "ed25519"}
CLS = {"P-256": T.CLS_P256, "P-384": T.CLS_P384, "P-521": T.CLS_P521, "Ed25519": T.CLS_ED25519}
TIERS = [(crv, w) for crv in ("P-256", "P-384", "P-521") for w in M.EC_WQ[CLS[crv]]] + \
        [("Ed25519", w) for w in M.ED_WA]
# one tier per curve whose build takes more than one slice
UNSLICED = [("P-256", 22), ("P-384", 20), ("P-521", 20), ("Ed25519", 22)]
_upgrader_digest = {}            # (curve, width) -> digest of the tier key's table as the tier test built it


def _fixtures():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "comb_tiers.json")))


def tier_key(crv, w):
    """the fixture key of a (curve, width) tier: tests/golden/comb_tiers.json, the tier's first key"""
    fx = _fixtures()
    if crv == "Ed25519":
        return fx["ed25519"]["keys"][0]
    return next(s for s in fx["ec"] if s["crv"] == crv and s["wq"] == w)["keys"][0]


def key_point(k):
    """the affine point a key's table is built from (Ed25519: -A; None: no table)"""
    if k["kty"] == "EC":
        return int(k["x"], 16), int(k["y"], 16)
    return T.ed_key_point(bytes.fromhex(k["x"]))


def check_table(ctx, key, cls, P, W):
    """geometry and the sample set of one table; returns the mismatches"""
    _, c, w, nwin, st = ctx.table_read(key)
    assert (c, w, nwin, st) == (cls, W, T.windows(cls, W), T.stride(cls))
    return T.table_mismatches(cls, P, W, nwin,
                              lambda first, count: ctx.table_read(key, first, count, out_words=count * st)[0])


def assert_exact(ctx, key, cls, P, W, label):
    t0 = time.time()
    bad = check_table(ctx, key, cls, P, W)
    print(f"[table-exact] {label}: check {time.time() - t0:.2f} s")
    assert not bad, (label, len(bad), bad[:8])


def load_at(ctx, keys, crv, w):
    """load `keys` (one curve) with the budget that buys exactly width w for each"""
    import bench
    from tests import gpu_helpers as H
    t0 = time.time()
    budget = len(keys) * bench.table_bytes(TAB[crv], w)
    assert bench.key_widths({TAB[crv]: len(keys)}, budget)[TAB[crv]] == w
    ctx.set_table_budget(budget)
    ctx.load_keys([H.abi_key(k) for k in keys])
    print(f"[table-exact] {crv} W = {w}: load of {len(keys)} key(s) {time.time() - t0:.2f} s")


def tier_table(crv, w, check):
    """The tier key's table at width w in a context of its own: `check` -> the
    sample mismatches, and the table's digest."""
    from cap_amd import _lib
    k = tier_key(crv, w)
    ctx = _lib.Context()
    try:
        load_at(ctx, [k], crv, w)
        assert ctx.table_widths() == [w]
        bad = check_table(ctx, 0, CLS[crv], key_point(k), w) if check else []
        return bad, ctx.table_digest(0)
    finally:
        ctx.close()


# ------------------------------------------------------------------ fixed-base tables
def test_generator_and_base_point_tables():
    from cap_amd import _lib
    from tests import gpu_helpers as H
    keys = [tier_key(crv, w) for crv, w in (("P-256", 20), ("P-384", 16), ("P-521", 16), ("Ed25519", 16))]
    ctx = _lib.Context()
    try:
        ctx.set_table_budget(0)                           # every key at its narrowest width
        t0 = time.time()
        ctx.load_keys([H.abi_key(k) for k in keys])
        print(f"[table-exact] fixed-base tables: load {time.time() - t0:.2f} s")
        assert ctx.table_widths() == [20, 16, 16, 16]
        for key, cls in ((_lib.TABLE_P256_G, T.CLS_P256), (_lib.TABLE_P384_G, T.CLS_P384),
                         (_lib.TABLE_P521_G, T.CLS_P521)):
            assert_exact(ctx, key, cls, T.ec_generator(cls), M.EC_WG[cls], f"generator table, class {cls}")
        assert_exact(ctx, _lib.TABLE_ED25519_B, T.CLS_ED25519, T.ed_base(), M.ED_WB, "Ed25519 base-point table")
    finally:
        ctx.close()


# ------------------------------------------------------------------ key tables, every tier
@pytest.mark.parametrize("crv,w", TIERS)
def test_key_table_tier(crv, w):
    t0 = time.time()
    bad, digest = tier_table(crv, w, check=True)
    print(f"[table-exact] {crv} W = {w}: whole case {time.time() - t0:.2f} s")
    assert not bad, (crv, w, len(bad), bad[:8])
    assert digest != 0
    _upgrader_digest[(crv, w)] = digest


# ------------------------------------------------------------------ unsliced builds
def _child():
    """CAPJWT_TABLES_SYNC=1: jg_keys_load itself builds each table at its
    budgeted width, in one launch.  Prints {"curve/width": {"bad": [...],
    "digest": n}} as the last line."""
    assert os.environ.get("CAPJWT_TABLES_SYNC") == "1"
    out = {}
    for crv, w in UNSLICED:
        bad, digest = tier_table(crv, w, check=True)
        out[f"{crv}/{w}"] = {"bad": [list(b) for b in bad[:8]], "nbad": len(bad), "digest": digest}
    print(json.dumps(out))


def test_unsliced_builds_equal_the_upgraders():
    env = dict(os.environ, CAPJWT_TABLES_SYNC="1")
    t0 = time.time()
    r = subprocess.run([sys.executable, "-u", "-m", "tests.test_gpu_table_exact"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    print(f"[table-exact] unsliced child: {time.time() - t0:.2f} s")
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(child) == sorted(f"{crv}/{w}" for crv, w in UNSLICED)
    for crv, w in UNSLICED:
        c = child[f"{crv}/{w}"]
        assert c["nbad"] == 0, (crv, w, c)
        if (crv, w) not in _upgrader_digest:              # run on its own: build the upgrader's table here
            _upgrader_digest[(crv, w)] = tier_table(crv, w, check=False)[1]
        assert c["digest"] == _upgrader_digest[(crv, w)] != 0, (crv, w)


# ------------------------------------------------------------------ several keys in one load
def _ed_key(y, sign=0):
    return {"kty": "OKP", "crv": "Ed25519", "x": (y | (sign << 255)).to_bytes(32, "little").hex()}


def _several(crv, w, keys):
    from cap_amd import _lib
    ctx = _lib.Context()
    try:
        load_at(ctx, keys, crv, w)
        assert ctx.table_widths() == [w, 0, w]
        with pytest.raises(_lib.JgError):
            ctx.table_read(1)
        with pytest.raises(_lib.JgError) as e:
            ctx.table_read(1, 0, 1, out_words=T.stride(CLS[crv]))
        assert set(e.value.words) == {_lib.TABLE_READ_FILL}
        assert ctx.table_digest(1) == 0
        for i in (0, 2):
            assert_exact(ctx, i, CLS[crv], key_point(keys[i]), w, f"{crv} W = {w}, key {i} of 3")
    finally:
        ctx.close()


def test_three_p256_keys_with_an_off_curve_one():
    fx = next(s for s in _fixtures()["ec"] if s["crv"] == "P-256" and s["wq"] == 20)["keys"]
    x, y = key_point(fx[2])
    off = dict(fx[2], y="%064x" % ((y + 1) % T.EC[T.CLS_P256]["p"]))
    assert not T.ec_on_curve(T.CLS_P256, key_point(off))
    _several("P-256", 20, [fx[0], off, fx[1]])


def test_three_ed25519_keys_with_an_undecodable_one():
    from tests import gpu_helpers as H
    y = next(y for y in range(2, 100) if key_point(_ed_key(y)) is None)
    ed_a = next(k for k in H.golden()[0] if k["kid"] == "ed-a")
    assert key_point(_ed_key(y)) is None                     # x^2 a non-square: SetBytes fails
    _several("Ed25519", 16, [tier_key("Ed25519", 16), _ed_key(y), ed_a])


# ------------------------------------------------------------------ Ed25519 edge keys
def _order8_y():
    """y of a point of order 8: the L-multiple of a curve point whose 4-multiple is not the identity"""
    for y in range(2, 100):
        A = T.ed_decode_key(y.to_bytes(32, "little"))
        if A is None:
            continue
        Q = T.ed_mul(T.ED_L, A)
        if T.ed_mul(4, Q) != T.ED_IDENTITY:
            assert T.ed_mul(8, Q) == T.ED_IDENTITY
            return Q
    raise AssertionError("no point of order 8 found")


def test_ed25519_edge_keys():
    """Go's SetBytes accepts every one of these encodings (y is reduced mod p,
    x = 0 takes either sign bit, and x^2 is a square for each), so each key
    has a table and every sampled entry equals the reference."""
    from cap_amd import _lib
    from tests import gpu_helpers as H
    p = T.ED_P
    q8 = _order8_y()
    keys = [("identity", _ed_key(1)), ("identity, sign bit set", _ed_key(1, 1)), ("y = p + 1", _ed_key(p + 1)),
            ("order 2", _ed_key(p - 1)), ("order 4", _ed_key(0)), ("order 8", _ed_key(q8[1], q8[0] & 1)),
            ("golden ed-a", next(k for k in H.golden()[0] if k["kid"] == "ed-a"))]
    pts = [key_point(k) for _, k in keys]
    assert pts[:5] == [(0, 1), (0, 1), (0, 1), (0, p - 1), (-T.ed_decode_key(bytes(32))[0] % p, 0)]
    assert pts[5] == (-q8[0] % p, q8[1]) and None not in pts
    assert T.ed_mul(2, pts[3]) == T.ED_IDENTITY != pts[3] and T.ed_mul(2, pts[4]) == pts[3]
    ctx = _lib.Context()
    try:
        load_at(ctx, [k for _, k in keys], "Ed25519", 16)
        assert ctx.table_widths() == [16] * len(keys)
        for i, (name, _) in enumerate(keys):
            assert_exact(ctx, i, T.CLS_ED25519, pts[i], 16, "Ed25519 W = 16, " + name)
        # the identity's Niels form, as stored
        assert T.ed_decode(ctx.table_read(0, 0, 1)[0]) == (1, 1, 0)
    finally:
        ctx.close()


# ------------------------------------------------------------------ the hook's refusals
def test_hook_refusals_copy_nothing():
    from cap_amd import _lib
    from tests import gpu_helpers as H
    rsa = next(k for k in H.golden()[0] if k["kty"] == "RSA")
    ctx = _lib.Context()
    try:
        ctx.set_table_budget(0)
        ctx.load_keys([H.abi_key(tier_key("P-256", 20)), H.abi_key(rsa)])
        assert ctx.table_widths() == [20, 0]
        st, total = 16, T.windows(T.CLS_P256, 20) << 19
        ok = ctx.table_read(0, total - 2, 2, out_words=2 * st)
        assert ok[1:] == (T.CLS_P256, 20, T.windows(T.CLS_P256, 20), st) and len(ok[0]) == 2 * st
        refused = [
            ("a key past the list", dict(key=2, first_entry=0, n_entries=1, out_words=st)),
            ("an unknown fixed-base table", dict(key=-5, first_entry=0, n_entries=1, out_words=st)),
            ("a key without a table (RSA)", dict(key=1, first_entry=0, n_entries=1, out_words=st)),
            ("a range past the end", dict(key=0, first_entry=total - 1, n_entries=2, out_words=2 * st)),
            ("a range that starts at the end", dict(key=0, first_entry=total, n_entries=1, out_words=st)),
            ("first_entry + n_entries past 2^64", dict(key=0, first_entry=2**64 - 1, n_entries=2, out_words=2 * st)),
            ("a short buffer", dict(key=0, first_entry=0, n_entries=2, out_words=2 * st - 1)),
            ("a fixed-base table not built yet", dict(key=_lib.TABLE_ED25519_B, first_entry=0, n_entries=1,
                                                      out_words=32)),
            ("a generator table past its end", dict(key=_lib.TABLE_P256_G, first_entry=10 << 25, n_entries=1,
                                                    out_words=st)),
        ]
        for name, kw in refused:
            with pytest.raises(_lib.JgError) as e:
                ctx.table_read(**kw)
            assert "rc=-1" in str(e.value) and "jg_debug_table_read" in str(e.value), name
            assert set(e.value.words) == {_lib.TABLE_READ_FILL}, name
        # the generator table this context did load is readable
        assert len(ctx.table_read(_lib.TABLE_P256_G, (10 << 25) - 1, 1)[0]) == st
    finally:
        ctx.close()


if __name__ == "__main__":
    _child()
