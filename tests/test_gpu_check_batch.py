"""Validator.CheckBatch / CheckBlob: the verdict-only entry whose registered
claims are scanned on the GPU (k_claims_scan), against ValidateBatch /
ValidateBlob token for token.

Tokens: the host_cases.json and tokens.json fixtures, and payloads of the
claims corpus (tests/claims_corpus.py) signed here with the committed test keys
(tests/craft.py, tests/golden/craft_keys.json).
"""
import base64
import json
import os

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import craft

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECOND = CC.SECOND
KID = "rsa2048-a"
SIG_PREFIX = "error verifying token signature: "


def b64u(b):
    return base64.urlsafe_b64encode(b).rstrip(b"=").decode()


def sign_rs256(payload_seg: str, header=None) -> str:
    """header.payload_seg.signature with the crafted rsa2048-a key (RS256)"""
    key = craft.keys()[KID]
    hdr = b64u(json.dumps(header or {"alg": "RS256", "kid": KID}, separators=(",", ":")).encode())
    si = (hdr + "." + payload_seg).encode()
    return hdr + "." + payload_seg + "." + b64u(craft.sign_raw(key, craft.pkcs1_em(key.k, 256, si)))


def tamper(tok: str) -> str:
    h, p, s = tok.split(".")
    return h + "." + p + "." + ("A" if s[0] != "A" else "B") + s[1:]


@pytest.fixture(scope="module")
def J():
    from cap_amd import jwt
    return jwt


@pytest.fixture(scope="module")
def crafted(J):
    """(validator over the crafted key, plain tokens + their segments, hard tokens)"""
    key = craft.keys()[KID]
    pub = J.PublicKey.rsa(key.n.to_bytes(key.k, "big"), key.e)
    ks, err = J.NewStaticKeySet([pub])
    assert err is None
    v, _ = J.NewValidator(ks)
    C = CC.corpus()
    plain = sorted({s for s, _ in C.plain})
    b64ok = lambda s: s and all(c in CC.B64 for c in s) and len(s) % 4 != 1
    hard = sorted({s for s, _ in C.hard + C.random[:600] if b64ok(s)})[::4]
    assert len(plain) > 100 and len(hard) > 100
    return (v, [sign_rs256(s.decode()) for s in plain], plain, [sign_rs256(s.decode()) for s in hard], hard, pub)


EXPECTED_SETS = [dict(), dict(CC.FULL), dict(CC.FULL, Issuer="other"), dict(Audiences=["b", "www.example.com"],
                                                                         ClockSkewLeeway=-1, ExpirationLeeway=-1)]


def E(J, ex, now_s, algs=("RS256",)):
    return J.Expected(Now=lambda: now_s, SigningAlgorithms=list(algs), **ex)


def test_plain_crafted_tokens_are_all_decided_on_the_device(crafted, J):
    v, toks, segs, _, _, _ = crafted
    seen = set()
    for ex in EXPECTED_SETS:
        for now_s in (CC.T0 + 30, CC.T0 + 700):
            e = E(J, ex, now_s)
            stats = {}
            got = v.CheckBatch(toks, e, stats)
            assert stats == {"scanned": len(toks), "host": 0}         # a scan that defers everything fails here
            assert got == [r[1] for r in v.ValidateBatch(toks, e)]
            exd = {k: (x * SECOND if k.endswith("Leeway") else x) for k, x in ex.items()}
            want = [_lib.CLAIM_ERRORS[CC.oracle_code(s, exd, now_s * SECOND)] for s in segs]
            assert got == want
            seen |= set(got)
    assert len(seen) >= 7, seen                      # accepts and most of the claim errors occur


def test_hard_crafted_tokens_match_validate_batch(crafted, J):
    v, _, _, toks, segs, _ = crafted
    want = []
    for ex in EXPECTED_SETS[:3]:
        e = E(J, ex, CC.T0 + 30)
        stats = {}
        got = v.CheckBatch(toks, e, stats)
        want = [r[1] for r in v.ValidateBatch(toks, e)]
        assert got == want
        assert stats["host"] > 20 and stats["scanned"] > 20
        # a segment with unused bits set is re-encoded by go-jose: the signature made over it here fails
        canon = [s for s in segs if CC.b64(base64.urlsafe_b64decode(s + b"=" * (-len(s) % 4))) == s]
        assert stats["scanned"] + stats["host"] == len(canon) < len(segs)
    assert any(w and w.startswith(SIG_PREFIX + "no known key") for w in want)     # a payload that is no JSON map


def test_blob_equals_validate_blob(crafted, J):
    v, plain, _, hard, _, _ = crafted
    toks = plain + hard + [tamper(t) for t in plain[:20]] + ["not-a-jwt", "a.b"]
    blob = "\n".join(toks).encode()
    for ex in EXPECTED_SETS[:2]:
        e = E(J, ex, CC.T0 + 30)
        stats = {}
        ok = v.CheckBlob(blob, e, stats)
        assert ok == v.ValidateBlob(blob, e)
        assert len(ok) == len(toks) and 0 < sum(ok) < len(ok)
        assert stats["scanned"] >= len(plain) and stats["host"] > 0


def test_signature_and_alg_errors_come_before_the_claims(crafted, J):
    v, plain, segs, _, _, _ = crafted
    e = E(J, dict(CC.FULL, Issuer="other"), CC.T0 + 30)
    bad = [tamper(t) for t in plain[:40]]
    got = v.CheckBatch(bad, e)
    assert got == [SIG_PREFIX + "no known key successfully validated the token signature"] * len(bad)
    assert got == [r[1] for r in v.ValidateBatch(bad, e)]
    # a verified token whose alg is not expected: the alg header error, whatever its claims say
    for algs in (("ES256",), ("ES256", "EdDSA"), (), ("HS256",)):
        e = E(J, dict(CC.FULL, Issuer="other"), CC.T0 + 30, algs=algs)
        got = v.CheckBatch(plain[:40] + bad[:5], e)
        assert got == [r[1] for r in v.ValidateBatch(plain[:40] + bad[:5], e)]
        if algs != ():
            assert all(g.startswith("invalid algorithm (alg) header parameter: ") for g in got[:40])
        assert all(g.startswith(SIG_PREFIX) for g in got[40:])
    # RS256 is Go's default allow-list
    e = J.Expected(Now=lambda: CC.T0 + 30)
    assert v.CheckBatch(plain[:40], e) == [r[1] for r in v.ValidateBatch(plain[:40], e)]
    assert v.CheckBatch([], e) == []


def test_fixture_tokens_match_validate_batch(golden, J):
    """The four Expected sets and three clocks of test_validate_batch_matches_validate_and_oracle."""
    from oracle import jws
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "host_cases.json")))
    kids = ["p256-a", "rsa2048-a", "ed-a", "p384-a"]
    nat = []
    for d in golden["keys_raw"]:
        if d["kid"] in kids:
            k = jws.Key.from_fixture(d)
            nat.append((kids.index(d["kid"]), J.PublicKey.rsa(k.n, k.e) if k.kty == "RSA" else
                        J.PublicKey.ec(k.crv, k.x, k.y) if k.kty == "EC" else J.PublicKey.ed25519(k.x)))
    ks, err = J.NewStaticKeySet([p for _, p in sorted(nat, key=lambda x: x[0])])
    assert err is None
    v, _ = J.NewValidator(ks)
    toks = [t["token"] for t in cases["tokens"]] + [t["token"] for t in golden["tokens"]]
    n_ok = 0
    for ex in [dict(SigningAlgorithms=["ES256", "RS256", "EdDSA", "PS256", "ES384"]),
               dict(SigningAlgorithms=["ES256"], Issuer="https://example.com/", Audiences=["www.example.com"]),
               dict(), dict(SigningAlgorithms=["ES256"], ClockSkewLeeway=-1, ExpirationLeeway=-1)]:
        for d in (1, 650, -300):
            e = J.Expected(Now=lambda: cases["t0"] + d, **ex)
            stats = {}
            got = v.CheckBatch(toks, e, stats)
            want = [r[1] for r in v.ValidateBatch(toks, e)]
            assert got == want, [(t[:50], g, w) for t, g, w in zip(toks, got, want) if g != w][:3]
            assert stats["scanned"] > 20 and stats["host"] > 5        # the fixtures hold both kinds
            n_ok += sum(g is None for g in got)
            one_line = [t for t in toks if "\n" not in t]
            blob = "\n".join(one_line).encode()
            assert v.CheckBlob(blob, e) == v.ValidateBlob(blob, e)
    assert n_ok > 50
    e = J.Expected(SigningAlgorithms=["ES256"], Now=lambda: cases["t0"])
    for tok in toks[:40]:
        assert v.CheckBatch([tok], e)[0] == v.Validate(tok, e)[1]


def test_jwks_keyset(crafted, J):
    from tests.test_gpu_edges import CountingJWKS
    _, plain, _, hard, _, _ = crafted
    key = craft.keys()[KID]
    jwk = {"kty": "RSA", "kid": KID, "n": b64u(key.n.to_bytes(key.k, "big")),
           "e": b64u(key.e.to_bytes(4, "big").lstrip(b"\0"))}
    ks, err = J.NewJSONWebKeySet(None, "https://check.example/jwks", "", CountingJWKS({"keys": [jwk]}, max_age=3600))
    assert err is None
    v, _ = J.NewValidator(ks)
    toks = plain[:60] + hard[:120] + [tamper(plain[0]), "x.y"]
    e = E(J, dict(CC.FULL), CC.T0 + 30)
    stats = {}
    # a cold key set verifies its first batch in the retry after the JWKS fetch, which
    # runs beside no scan: every token takes the host path, with the same results
    assert v.CheckBatch(toks, e, stats) == [r[1] for r in v.ValidateBatch(toks, e)]
    assert stats["scanned"] == 0 and stats["host"] > 60
    assert v.CheckBatch(toks, e, stats) == [r[1] for r in v.ValidateBatch(toks, e)]
    assert stats["scanned"] >= 60
