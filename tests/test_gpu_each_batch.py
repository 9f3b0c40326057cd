"""Validator.CheckBatchEach / RegisteredBatchEach / SelectBatchEach and their
*BlobEach forms: an Expected per token, one signature submission and one GPU
scan (k_claims_*_each) for a batch of several tenants.  Every result must be
what the existing entry returns for that token's profile group -- and what
ValidateBatch returns for it: accept, error and the claim values.

About 300 tokens of three tenants whose profiles differ in issuer, audiences,
Now and SigningAlgorithms, a profile with 17 audiences (no device slot: the host
path) and one that takes no alg the tokens carry; wrong-tenant tokens, tokens
expired under one profile's clock only, payloads the scan leaves to the host,
tampered signatures.  Tokens are crafted as tests/test_gpu_registered_batch.py
crafts them, signed with the committed test key (tests/craft.py).
"""
import array
import json

import pytest

from tests import claims_corpus as CC
from tests import claims_select_cases as SC
from tests import craft
from tests.test_gpu_check_batch import KID, SIG_PREFIX, sign_rs256, tamper
from tests.test_gpu_registered_batch import unpack_blob
from tests.test_gpu_select_batch import blob_values

pytestmark = pytest.mark.gpu

T0 = CC.T0
NAMES = ["scope", "roles", "n", "missing"]
ISS = ["https://a.example/", "https://b.example/", "https://c.example/", "https://wide.example/",
       "https://a.example/"]
AUD = ["client-a", "client-b2", "client-c", "aud-16", "client-a"]
WIDE, NOALG = 3, 4


@pytest.fixture(scope="module")
def J():
    from cap_amd import jwt
    return jwt


@pytest.fixture(scope="module")
def profiles(J):
    def P(iss, aud, now_s, algs, **kw):
        return J.Expected(Issuer=iss, Audiences=aud, Now=lambda: now_s, SigningAlgorithms=algs, **kw)
    return [
        P(ISS[0], ["client-a"], T0 + 30, ["RS256"]),
        P(ISS[1], ["client-b", "client-b2"], T0 + 30, ["ES256", "RS256"], ClockSkewLeeway=5),
        P(ISS[2], ["client-c"], T0 + 1000, ["RS256"]),                     # a later clock: exp T0 + 600 is over
        P(ISS[3], ["aud-%d" % k for k in range(17)], T0 + 30, ["RS256"]),  # 17 audiences: no device slot
        P(ISS[4], ["client-a"], T0 + 30, ["ES256"]),                       # the tokens' alg is not expected
    ]


def payload(iss, aud, exp, k, **more):
    d = {"iss": iss, "aud": [aud, "other"], "exp": exp, "iat": T0, "sub": "user-%d" % k, "scope": "read write",
         "roles": ["r%d" % k, {"k": [k]}], "n": k + 0.5}
    d.update(more)
    return CC.js(d)


@pytest.fixture(scope="module")
def batch(J):
    """(validator, tokens, which)"""
    key = craft.keys()[KID]
    ks, err = J.NewStaticKeySet([J.PublicKey.rsa(key.n.to_bytes(key.k, "big"), key.e)])
    assert err is None
    v, _ = J.NewValidator(ks)
    toks, which = [], []
    for k in range(60):
        for p in range(5):                                   # neighbouring tokens of different profiles
            o = (p + 1) % 3
            kind = k % 12
            if kind < 4:
                raw = payload(ISS[p], AUD[p], T0 + 1600, k)                       # valid for its own profile
            elif kind == 4:
                raw = payload(ISS[o], AUD[p], T0 + 1600, k)                       # another tenant's issuer
            elif kind == 5:
                raw = payload(ISS[p], AUD[o] + "x", T0 + 1600, k)                 # no audience of this profile
            elif kind == 6:
                raw = payload(ISS[p], AUD[p], T0 + 600, k)                        # expired under profile 2's clock alone
            elif kind == 7:
                raw = payload(ISS[p], AUD[p], T0 + 1600, k).replace(b'"read write"', b'"read\\u0020write"')   # an escape
            elif kind == 8:
                raw = payload(ISS[p], AUD[p], T0 + 1600, k)[:-1] + b',"EXP":1}'   # a field twice
            elif kind == 9:
                raw = payload(ISS[p], AUD[p], T0 + 1600, k, nbf="soon")           # rejected by the host path
            elif kind == 10:
                raw = payload(ISS[p], AUD[p], T0 - 600, k)                        # expired for all
            else:
                raw = CC.js({"sub": "no dates"})
            tok = sign_rs256(CC.b64(raw).decode())
            toks.append(tamper(tok) if k % 15 == 14 else tok)
            which.append(p)
    toks += ["not-a-jwt", "a.b"]
    which += [1, 2]
    assert len(toks) == 302
    return v, toks, which


def per_group(toks, which, nprof, call):
    """call(tokens of profile p, p) per profile, scattered back into token order"""
    out = [None] * len(toks)
    for p in range(nprof):
        at = [i for i, w in enumerate(which) if w == p]
        for i, r in zip(at, call([toks[i] for i in at], p)):
            out[i] = r
    return out


def test_each_entries_equal_the_existing_ones_and_validate_batch(batch, profiles, J):
    v, toks, which = batch
    n = len(profiles)
    full = per_group(toks, which, n, lambda t, p: v.ValidateBatch(t, profiles[p]))
    gstats = []

    def check_group(t, p):
        st = {}
        out = v.CheckBatch(t, profiles[p], st)
        gstats.append(st)
        return out
    want_c = per_group(toks, which, n, check_group)
    want_r = per_group(toks, which, n, lambda t, p: v.RegisteredBatch(t, profiles[p]))
    want_s = per_group(toks, which, n, lambda t, p: v.SelectBatch(t, NAMES, profiles[p]))
    sc, sr, ss = {}, {}, {}
    errs = v.CheckBatchEach(toks, profiles, which, sc)
    rows = v.RegisteredBatchEach(toks, profiles, which, sr)
    sels = v.SelectBatchEach(toks, NAMES, profiles, which, ss)
    assert errs == want_c == [r[1] for r in full]
    assert rows == want_r
    assert [(r[0], r[2]) for r in sels] == [(r[0], r[2]) for r in want_s] == rows
    for (claims, values, err), (m, _), w in zip(sels, full, want_s):
        if err is None:
            assert SC.same(values, {k: m[k] for k in NAMES if k in m}) and SC.same(values, w[1])
            assert claims["sub"] == m["sub"] and claims["exp"] == m["exp"] and claims["iss"] == m["iss"]
            assert claims["aud"] == m["aud"]
        else:
            assert claims is None and values is None
    # the same tokens, the same paths: the groups' counts add up (the 17-audience profile is host in both)
    assert sc == sr == ss
    assert sc["scanned"] == sum(s["scanned"] for s in gstats) > 100
    assert sc["host"] == sum(s["host"] for s in gstats) > 30
    # what the batch is made of
    by = lambda p, pred: sum(1 for e, w in zip(errs, which) if w == p and pred(e))
    assert all(by(p, lambda e: e is None) >= 20 for p in range(4))
    assert by(NOALG, lambda e: e is None) == 0
    assert by(NOALG, lambda e: e and "token signed with unexpected algorithm" in e) >= 50
    assert by(2, lambda e: e and "token is expired" in e) > by(0, lambda e: e and "token is expired" in e) > 0
    assert all(by(p, lambda e: e == "invalid issuer (iss) claim") == 5 for p in range(4))
    assert sum(1 for e in errs if e and e.startswith(SIG_PREFIX)) >= 20


def test_the_profile_without_a_slot_answers_through_the_host(batch, profiles):
    v, toks, which = batch
    at = [i for i, w in enumerate(which) if w == WIDE]
    mine = [toks[i] for i in at]
    alone = {}
    want = v.CheckBatch(mine, profiles[WIDE], alone)
    assert alone["scanned"] == 0 and alone["host"] > 40            # not scannable today either
    # ... and with the three tenants in front of it: scanned tokens beside it, its own on the host
    st = {}
    got = v.CheckBatchEach(toks, profiles, which, st)
    assert [got[i] for i in at] == want and want.count(None) >= 20
    only = {}
    v.CheckBatchEach(mine, profiles, [WIDE] * len(mine), only)
    assert only == alone
    assert st["scanned"] > 100 and st["host"] >= alone["host"]


def test_blob_forms_equal_the_batch_rows(batch, profiles):
    v, toks, which = batch
    blob = "\n".join(toks).encode()
    w32 = array.array("I", which)
    assert w32.itemsize == 4
    sb, sr, ss, st = {}, {}, {}, {}
    ok = v.CheckBlobEach(blob, profiles, w32, sb)
    errs = v.CheckBatchEach(toks, profiles, which, st)
    assert ok == bytes(e is None for e in errs) and 0 < sum(ok) < len(ok)
    groups = per_group(toks, which, len(profiles), lambda t, p: v.CheckBlob("\n".join(t).encode(), profiles[p]))
    assert ok == bytes(groups)
    cols = v.RegisteredBlobEach(blob, profiles, w32, sr)
    rows = v.RegisteredBatchEach(toks, profiles, which)
    assert cols["ok"] == ok and unpack_blob(cols, len(toks)) == [r[0] for r in rows]
    scols = v.SelectBlobEach(blob, NAMES, profiles, w32, ss)
    srows = v.SelectBatchEach(toks, NAMES, profiles, which)
    assert scols["ok"] == ok and unpack_blob(scols, len(toks)) == [r[0] for r in srows]
    got = blob_values(scols, NAMES, len(toks))
    assert all((g is None) == (r[1] is None) for g, r in zip(got, srows))
    assert all(SC.same(g, r[1]) for g, r in zip(got, srows) if g is not None)
    assert sb == sr == ss == st and st["scanned"] > 0
    # one profile for every token: the old blob entry
    zeros = array.array("I", [0] * len(toks))
    assert v.CheckBlobEach(blob, profiles[1:2], zeros) == v.CheckBlob(blob, profiles[1])


def test_argument_errors(batch, profiles):
    v, toks, which = batch
    blob = "\n".join(toks).encode()
    with pytest.raises(ValueError):
        v.CheckBatchEach(toks, profiles, which[:-1])
    with pytest.raises(ValueError):
        v.RegisteredBatchEach(toks, profiles, which[:5] + [len(profiles)] + which[6:])
    with pytest.raises(ValueError):
        v.SelectBatchEach(toks, NAMES, [], which)
    with pytest.raises(ValueError):
        v.CheckBlobEach(blob, profiles, array.array("I", which[:-1]))
    with pytest.raises(ValueError):
        v.CheckBlobEach(blob, profiles, array.array("B", [0] * len(toks)))       # not uint32
    with pytest.raises(ValueError):
        v.SelectBlobEach(blob, NAMES, profiles, array.array("I", [9] * len(toks)))
    assert v.CheckBatchEach([], [], []) == []
    assert json.dumps(v.CheckBatchEach(toks[:3], profiles, which[:3])) == json.dumps(
        [v.CheckBatch([t], profiles[w])[0] for t, w in zip(toks[:3], which[:3])])
