"""Validator.MatchBatchArgs / MatchBlobArgs and their *Each forms with hash
columns: at_hash against the request's access token and c_hash against its
authorization code, hashed and encoded on the device (k_hash_operand) and compared
by the scan (k_claims_match_args), beside the request's own nonce.

Tokens are crafted and signed with the committed test keys (tests/craft.py):
RS256, RS384 and RS512 through pkcs1_em, EdDSA through ed_sign; each carries
at_hash, c_hash and nonce.  ok / err are ValidateBatch's; IsString & HashOfEach is
the `verified` of oracle.oidc.verify_access_token / verify_authorization_code,
token for token, and Go's error case (a hash mismatch) is IsString & not
HashOfEach under an alg other than EdDSA.
"""
import json
import struct

import pytest

from oracle import oidc
from tests import claims_corpus as CC
from tests import claims_match_hash_cases as HC
from tests import craft
from tests.test_gpu_check_batch import KID, b64u, tamper

pytestmark = pytest.mark.gpu
ALGS = ("RS256", "RS384", "RS512", "EdDSA")
FAM = {"RS256": 1, "RS384": 2, "RS512": 3}
KINDS = ["correct"] * 9 + ["wrong"] * 3 + ["absent", "number", "null", "empty", "eddsa", "eddsa", "none", "none", "big", "escape",
                                           "escape", "expired", "tampered", "wrong-code"]


@pytest.fixture(scope="module")
def J():
    from cap_amd import jwt
    return jwt


def sign(alg, payload: bytes) -> str:
    hdr = b64u(json.dumps({"alg": alg, "kid": KID if alg != "EdDSA" else "ed-a"}, separators=(",", ":")).encode())
    si = (hdr + "." + CC.b64(payload).decode()).encode()
    if alg == "EdDSA":
        sig = craft.ed_sign(craft.keys()["ed-a"], si)
    else:
        key = craft.keys()[KID]
        sig = craft.sign_raw(key, craft.pkcs1_em(key.k, int(alg[2:]), si))
    return si.decode() + "." + b64u(sig)


def access_token(k, kind):
    return b"t" * 8193 if kind == "big" else b"ya29.a0Af_%04d-" % k + HC.source(k, 24).hex().encode()


@pytest.fixture(scope="module")
def crafted(J):
    """(validator, tokens, kinds, algs, nonces, access tokens, codes): the columns the requests would hold"""
    key = craft.keys()[KID]
    ks, err = J.NewStaticKeySet([J.PublicKey.rsa(key.n.to_bytes(key.k, "big"), key.e),
                                 J.PublicKey.ed25519(craft.ed_public(craft.keys()["ed-a"])[2])])
    assert err is None
    v, _ = J.NewValidator(ks)
    kinds = [KINDS[(5 * k) % len(KINDS)] for k in range(len(KINDS))]             # interleaved
    toks, algs, nonces, ats, codes = [], [], [], [], []
    for k, kind in enumerate(kinds):
        alg = "EdDSA" if kind == "eddsa" else ALGS[k % 3]
        fam = FAM.get(alg, 1)                                                    # an EdDSA token still carries some at_hash
        at, code = access_token(k, kind), b"SplxlOBeZQQYbYS6WxSbIA-%d" % k
        claims = {"iss": "https://example.com/", "aud": "www.example.com", "sub": "alice@example.com", "iat": CC.T0,
                  "exp": CC.T0 + (-600 if kind == "expired" else 600), "nonce": "n-%d" % k,
                  "at_hash": HC.hash_value(at, fam).decode(), "c_hash": HC.hash_value(code, fam).decode()}
        if kind == "absent":
            del claims["at_hash"]
        elif kind in ("number", "null", "empty"):
            claims["at_hash"] = {"number": 7, "null": None, "empty": ""}[kind]
        payload = json.dumps(claims, separators=(",", ":")).encode()
        if kind == "escape":
            payload = payload.replace(b'"alice@example.com"', b'"alice\\u0040example.com"')
        t = sign(alg, payload)
        toks.append(tamper(t) if kind == "tampered" else t)
        algs.append(alg)
        nonces.append("n-%d" % (k if k % 7 else k + 1))
        ats.append(None if kind == "none" else AC_flip(at) if kind == "wrong" else at)
        codes.append(AC_flip(code) if kind == "wrong-code" else code)
    return v, toks, kinds, algs, nonces, ats, codes


def AC_flip(v):
    return (b"A" if v[:1] != b"A" else b"B") + v[1:]


def requires(J):
    return [J.EqualsEach("nonce", 0), J.HashOfEach("at_hash", 0), J.IsString("at_hash"), J.HashOfEach("c_hash", 1),
            J.IsString("c_hash")]


def expected(J, now_s=CC.T0 + 30):
    return J.Expected(Now=lambda: now_s, SigningAlgorithms=list(ALGS), Issuer="https://example.com/")


def check_rows(v, J, crafted, rows, e):
    _, toks, kinds, algs, nonces, ats, codes = crafted
    full = v.ValidateBatch(toks, e)
    assert [r[1] for r in rows] == [r[1] for r in full] == v.CheckBatch(toks, e)
    hits = errs = 0
    for i, ((bits, err), kind) in enumerate(zip(rows, kinds)):
        assert (err is None) == (kind not in ("expired", "tampered")), (i, kind, err)
        if err is not None:
            assert bits is None
            continue
        assert bits & 1 == (nonces[i] == "n-%d" % i), i
        for claim, col, b in (("at_hash", ats, 1), ("c_hash", codes, 3)):
            hash_of, is_str = (bits >> b) & 1, (bits >> (b + 1)) & 1
            if col[i] is None:
                assert hash_of == 0 and is_str == 1, (i, kind)
                continue
            verified, go_err = oidc.verify_hash_claim(claim, toks[i], col[i])
            assert bool(is_str & hash_of) == verified, (i, kind, claim, bits)
            assert hash_of <= is_str
            # Go's err != nil: the claim is a string, the hash differs, the alg is not EdDSA
            assert (go_err == "mismatch") == bool(is_str and not hash_of and algs[i] != "EdDSA"), (i, kind, claim, go_err)
            assert go_err in (None, "mismatch")
            hits += verified
            errs += go_err == "mismatch"
    assert hits >= 20 and errs >= 4
    return [b for b, _ in rows]


def test_hash_claims_are_checked_on_the_device(crafted, J):
    v, toks, kinds, algs, nonces, ats, codes = crafted
    reqs, e = requires(J), expected(J)
    stats = {}
    rows = v.MatchBatchArgs(toks, reqs, [nonces], [], e, stats, hashes=[ats, codes])
    verified = sum(k != "tampered" for k in kinds)
    host = sum(k in ("escape", "big") for k in kinds)
    assert stats == {"scanned": verified - host, "host": host}                   # everything else was decided on the device
    bits = check_rows(v, J, crafted, rows, e)
    for i, kind in enumerate(kinds):
        if kind in ("correct", "big", "escape"):
            assert bits[i] | 1 == 0b11111, (i, kind, bits[i])
        if kind in ("absent", "number", "null"):
            assert bits[i] & 0b110 == 0 and bits[i] >> 3 == 0b11, (i, kind)
        if kind in ("empty", "eddsa", "none", "wrong"):
            assert bits[i] & 0b110 == 0b100, (i, kind, bits[i])
        if kind == "eddsa":
            assert bits[i] >> 1 == 0b1010
        if kind == "wrong-code":
            assert bits[i] >> 1 == 0b1011
    assert {a for a, k in zip(algs, kinds) if k == "correct"} == {"RS256", "RS384", "RS512"}
    # str entries, and the columns the other way round with the requirements renumbered
    assert v.MatchBatchArgs(toks, reqs, [nonces], [], e, hashes=[[a if a is None else a.decode() for a in ats], codes]) == rows
    swapped = [reqs[0], J.HashOfEach("at_hash", 1), reqs[2], J.HashOfEach("c_hash", 0), reqs[4]]
    assert v.MatchBatchArgs(toks, swapped, [nonces], [], e, hashes=[codes, ats]) == rows
    # IsString alone needs no column
    only = v.MatchBatchArgs(toks, [reqs[2], reqs[4]], expected=e)
    assert [b for b, _ in only] == [None if b is None else (b >> 2 & 1) | (b >> 4 & 1) << 1 for b in bits]
    assert v.MatchBatchArgs([], reqs, [[]], [], e, hashes=[[], []]) == []


def test_lists_over_the_caps_and_what_throws(crafted, J):
    v, toks, kinds, algs, nonces, ats, codes = crafted
    reqs, e = requires(J), expected(J)
    want = v.MatchBatchArgs(toks, reqs, [nonces], [], e, hashes=[ats, codes])
    verified = sum(k != "tampered" for k in kinds)
    for strs, hashes in (([nonces], [ats, codes, ats]), ([nonces] * 3, [ats, codes])):
        stats = {}
        assert v.MatchBatchArgs(toks, reqs, strs, [], e, stats, hashes=hashes) == want      # results never depend on the caps
        assert stats == {"scanned": 0, "host": verified}
    for call in (lambda: v.MatchBatchArgs(toks, reqs, [nonces], [], e, hashes=[ats[:-1], codes]),
                 lambda: v.MatchBatchArgs(toks, reqs, [nonces], [], e, hashes=[ats]),
                 lambda: v.MatchBatchArgs(toks, reqs, [nonces], [], e),
                 lambda: v.MatchBatchArgs(toks, reqs + [J.HashOfEach("x", 2)], [nonces], [], e, hashes=[ats, codes]),
                 lambda: v.MatchBlobArgs("\n".join(toks).encode(), reqs, [b"\n".join(n.encode() for n in nonces)], [], e,
                                         hashes=[b"only-one", b"x"])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        v.MatchBatchArgs(toks[:1], reqs, [nonces[:1]], [], e, hashes=[[5], [b"x"]])
    with pytest.raises(TypeError):
        v.MatchBatch(toks[:1], [J.IsString("a")], e)                            # the MatchBatch family takes its own four alone
    assert repr(J.HashOfEach("at_hash", 1)) == "HashOfEach(%r, 1)" % (J.Path("at_hash"),) and "IsString" in repr(J.IsString("a"))


def masks_of(cols, n):
    assert len(cols["ok"]) == n and len(cols["match"]) == 4 * n
    return list(struct.unpack("<%dI" % n, cols["match"]))


def test_blob_and_each_forms_equal_the_batch_rows(crafted, J):
    v, toks, kinds, algs, nonces, ats, codes = crafted
    toks = toks + ["not-a-jwt"]
    nonces, ats, codes = nonces + [""], ats + [None], codes + [b"c"]
    blob = "\n".join(toks).encode()
    col = lambda c: b"\n".join(b"" if x is None else x for x in c)
    reqs, e = requires(J), expected(J)
    stats, bstats = {}, {}
    rows = v.MatchBatchArgs(toks, reqs, [nonces], [], e, stats, hashes=[ats, codes])
    cols = v.MatchBlobArgs(blob, reqs, ["\n".join(nonces).encode()], [], e, bstats, hashes=[col(ats), col(codes)])
    assert sorted(cols) == ["match", "ok"] and cols["ok"] == v.CheckBlob(blob, e)
    assert bstats == stats and stats["host"] > 0 and stats["scanned"] > 0
    assert masks_of(cols, len(toks)) == [b or 0 for b, _ in rows]
    assert list(cols["ok"]) == [int(err is None) for _, err in rows]
    assert ats[-1] is None and col(ats).endswith(b"\n")                         # the last entry is an empty line: no value
    assert v.MatchBlobArgs(blob, reqs, ["\n".join(nonces).encode()], [], e, hashes=[col(ats) + b"\n", col(codes)]) == cols
    # an Expected per token: each row is its own Expected's
    es = [e, expected(J, CC.T0 + 7200), J.Expected(Now=lambda: CC.T0 + 30, SigningAlgorithms=list(ALGS), Issuer="other")]
    which = [i % 3 for i in range(len(toks))]
    estats = {}
    each = v.MatchBatchArgsEach(toks, reqs, es, which, [nonces], [], estats, hashes=[ats, codes])
    alone = [v.MatchBatchArgs(toks, reqs, [nonces], [], x, hashes=[ats, codes]) for x in es]
    assert each == [alone[w][i] for i, w in enumerate(which)]
    assert [err for _, err in each] == v.CheckBatchEach(toks, es, which)
    assert estats["scanned"] > 0 and estats["host"] > 0 and 0 < sum(err is None for _, err in each) < len(toks) - 3
    import array
    ecols = v.MatchBlobArgsEach(blob, reqs, es, array.array("I", which), ["\n".join(nonces).encode()], [],
                                hashes=[col(ats), col(codes)])
    assert masks_of(ecols, len(toks)) == [b or 0 for b, _ in each]
    assert list(ecols["ok"]) == [int(err is None) for _, err in each]
