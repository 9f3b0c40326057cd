"""The big-integer model of the scalar-level stages (tests/scalar_model.py), held
to itself, to the kernels' constants and to oracle.jws (no GPU): the exact GPU
tests (test_gpu_ec_scalar_exact.py, test_gpu_ed_exact.py) compare the device
with this model, so it must not share a mistake with the kernels."""
import hashlib
import json
import os
import random
import re

import pytest

from oracle import jws
from tests import scalar_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASH = {M.ES256: hashlib.sha256, M.ES384: hashlib.sha384, M.ES512: hashlib.sha512}


def _limbs_const(struct, name):
    src = open(os.path.join(ROOT, "cap_amd", "csrc", "kernels", "field_consts.hpp")).read()
    body = re.search(r"struct %s \{(.*?)\n\};" % struct, src, re.S).group(1)
    vals = re.search(r"uint32_t %s\[L\] = \{([^}]*)\}" % name, body).group(1)
    return sum(int(v.strip().rstrip("u"), 16) << (28 * i) for i, v in enumerate(vals.split(",")))


def test_orders_are_the_kernels():
    assert _limbs_const("P256N", "M") == M.EC_N[M.CLS_P256]
    assert _limbs_const("P384N", "M") == M.EC_N[M.CLS_P384]
    assert _limbs_const("P521N", "M") == M.EC_N[M.CLS_P521]
    assert _limbs_const("ED25519L", "M") == M.ED_L
    assert _limbs_const("ED25519P", "M") == M.ED_P
    for cls, n in M.EC_N.items():
        assert n.bit_length() == M.EC_BITS[cls]


def _edge_scalars(n, bits, w, rng):
    half, full = 1 << (w - 1), (1 << w) - 1
    k = (bits - 1) // w
    us = [0, 1, half - 1, half, half + 1, n - 1, n - 2, n >> 1]
    us += [sum(v << (w * i) for i in range(k)) for v in (half - 1, half, half + 1, full)]
    us += [(n >> (w * k) << (w * k)) | (half << (w * (k - 1)))]
    us += [rng.randrange(n) for _ in range(200)]
    return [u for u in us if 0 <= u < n]


def test_ecdsa_recoding_reconstructs_and_stays_in_range():
    rng = random.Random(1)
    for cls, n in M.EC_N.items():
        for w in set(M.EC_WQ[cls]) | {M.EC_WG[cls]}:
            nwin = M.ec_windows(cls, w)
            for u in _edge_scalars(n, M.EC_BITS[cls], w, rng):
                d, c = M.recode(u, w, nwin, True)
                assert c == 0 and M.digits_value(d, w) == u
                assert all(-(1 << (w - 1)) <= x < (1 << (w - 1)) for x in d)


def test_ed25519_recoding_reconstructs_and_stays_in_range():
    rng = random.Random(2)
    for w in set(M.ED_WA) | {M.ED_WB}:
        nwin = M.ed_windows(w)
        for u in _edge_scalars(M.ED_L, 253, w, rng):
            d, c = M.recode(u, w, nwin, False)
            assert c == 0 and M.digits_value(d, w) == u
            assert all(-(1 << (w - 1)) < x <= (1 << (w - 1)) for x in d)
    # the two rules differ exactly at a window of 2^(W-1)
    assert M.recode(1 << 15, 16, 2, True)[0] == [-(1 << 15), 1]
    assert M.recode(1 << 15, 16, 2, False)[0] == [1 << 15, 0]


def _ecdsa_tokens():
    d = os.path.join(ROOT, "tests", "golden")
    edge = json.load(open(os.path.join(d, "ec_edge.json")))
    out = [(t, {k["kid"]: k for k in edge["keys"]}, None) for t in edge["tokens"] if t["alg"].startswith("ES")]
    for s in json.load(open(os.path.join(d, "comb_tiers.json")))["ec"]:
        out += [(t, {k["kid"]: k for k in s["keys"]}, s) for t in s["tokens"]]
    return out


def test_reject_rule_and_digits_agree_with_the_oracle_and_the_fixtures():
    seen_rej = seen_acc = 0
    for t, keys, tier in _ecdsa_tokens():
        p = jws.parse_jws(t["token"])
        key = keys[t["key"]]
        cls, alg = M.EC_CLS[key["crv"]], jws.ALGS[p.alg]
        want = jws.verify_sig(p, jws.Key.from_fixture(key))
        assert int(want) == t["verdict"], t["name"]
        sz = M.ES_SIZE[alg]
        assert len(p.signature) == 2 * sz, t["name"]
        r, s = int.from_bytes(p.signature[:sz], "big"), int.from_bytes(p.signature[sz:], "big")
        u = M.ec_scalars(cls, alg, r, s, HASH[alg](p.signing_input).digest())
        if u is None:
            seen_rej += 1
            assert not want, t["name"]               # the model rejects: so does crypto/ecdsa.Verify
            continue
        seen_acc += 1
        if tier is not None and t["verdict"]:
            # the fixture records the digits its generator crafted the token for
            wg, wq = tier["wg"], tier["wq"]
            assert M.recode(u[0], wg, M.ec_windows(cls, wg), True)[0] == t["u1_digits"], t["name"]
            assert M.recode(u[1], wq, M.ec_windows(cls, wq), True)[0] == t["u2_digits"], t["name"]
    assert seen_acc > 100


@pytest.mark.parametrize("cls", [M.CLS_P256, M.CLS_P384, M.CLS_P521])
def test_range_rule_against_the_oracle(cls):
    """signatures with r or s at the ends of the range, on a fixture key: where
    the model rejects, the C oracle (crypto/ecdsa.Verify restated) returns false"""
    crv = {v: k for k, v in M.EC_CLS.items()}[cls]
    edge = json.load(open(os.path.join(ROOT, "tests", "golden", "ec_edge.json")))
    key = jws.Key.from_fixture(next(k for k in edge["keys"] if k["crv"] == crv))
    n, alg = M.EC_N[cls], {M.CLS_P256: "ES256", M.CLS_P384: "ES384", M.CLS_P521: "ES512"}[cls]
    sz = M.ES_SIZE[jws.ALGS[alg]]
    msg = b"signing.input"
    for r, s in ((0, 5), (5, 0), (n, 5), (5, n), (n + 1, 5), (5, n + 1), ((1 << (8 * sz)) - 1, 5), (5, (1 << (8 * sz)) - 1)):
        assert M.ec_scalars(cls, jws.ALGS[alg], r, s, HASH[jws.ALGS[alg]](msg).digest()) is None
        assert not jws.verify_alg_sig(alg, key, msg, r.to_bytes(sz, "big") + s.to_bytes(sz, "big"))
    for r, s in ((1, n - 1), (n - 1, 1)):
        assert M.ec_scalars(cls, jws.ALGS[alg], r, s, HASH[jws.ALGS[alg]](msg).digest()) is not None


def test_ed_model_against_the_craft_reference():
    from tests import craft
    assert (M.ED_P, M.ED_L) == (craft.ED_P, craft.ED_L)
    rng = random.Random(3)
    for _ in range(20):
        seed, msg = bytes(rng.randrange(256) for _ in range(32)), bytes(rng.randrange(256) for _ in range(40))
        sig, pub = craft.ed_sign(seed, msg), craft.ed_public(seed)[2]
        assert M.ed_s_ok(sig[32:])
        k = M.ed_k(hashlib.sha512(sig[:32] + pub + msg).digest())
        # R = [S]B - [k]A, encoded, is sig[:32]
        A = (craft._ed_recover_x(int.from_bytes(pub, "little") & ((1 << 255) - 1), pub[31] >> 7),
             int.from_bytes(pub, "little") & ((1 << 255) - 1))
        negA = ((-A[0]) % M.ED_P, A[1], 1, (-A[0]) * A[1] % M.ED_P)
        R = craft._ed_add(craft._ed_mul(int.from_bytes(sig[32:], "little"), craft.ED_B), craft._ed_mul(k, negA))
        assert M.ed_encode(R[0], R[1], R[2]) == sig[:32]
    assert not M.ed_s_ok(M.ED_L.to_bytes(32, "little"))
    assert M.ed_s_ok((M.ED_L - 1).to_bytes(32, "little"))
    assert not M.ed_s_ok((1 << 253).to_bytes(32, "little"))
