"""Validator.MatchBatch / MatchBlob / MatchBatchEach / MatchBlobEach: yes/no
questions about claims answered by the GPU scan (k_claims_match_each), against
CheckBatch and ValidateBatch for the errors and a plain-Python evaluation of the
requirements on ValidateBatch's claims map for the bits.

Tokens are crafted as tests/test_gpu_paths_batch.py crafts them: Keycloak-style
payloads, the directed list of tests/claims_match_cases.py and a slice of the
claims corpus, signed with the committed test key (tests/craft.py).  Payloads
with an escape take the host path.
"""
import array
import struct

import pytest

from tests import claims_corpus as CC
from tests import claims_match_cases as MC
from tests import craft
from tests.test_gpu_check_batch import E, EXPECTED_SETS, KID, sign_rs256, tamper
from tests.test_gpu_paths_batch import keycloak

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def J():
    from cap_amd import jwt
    return jwt


@pytest.fixture(scope="module")
def crafted(J):
    """(validator, tokens the scan decides, tokens it leaves to the host)"""
    key = craft.keys()[KID]
    ks, err = J.NewStaticKeySet([J.PublicKey.rsa(key.n.to_bytes(key.k, "big"), key.e)])
    assert err is None
    v, _ = J.NewValidator(ks)
    C = CC.corpus()
    plain = ([CC.b64(keycloak(k)) for k in range(40)] + sorted({s for s, _, _ in MC.directed()})
             + sorted({s for s, _ in C.plain})[::6])
    hard = [CC.b64(keycloak(k, escape=True)) for k in range(12)]
    return v, [sign_rs256(s.decode()) for s in plain], [sign_rs256(s.decode()) for s in hard]


def keycloak_requires(J):
    P = J.Path
    return [J.HasElement(P("realm_access", "roles"), "role-3"), J.HasElement(P("realm_access", "roles"), "uma_authorization"),
            J.HasElement(P("realm_access", "roles"), "realm/admin"), J.HasWord("scope", "email"), J.HasWord("scope", "mail"),
            J.Equals("scope", "openid email"), J.Present(P("cnf", "jkt")), J.Present(P("cnf", "x5t#S256")),
            J.Equals(P("act", "sub"), "svc-7"), J.HasElement(P("resource_access", "app", "roles"), "r5"),
            J.Present(P("a", "b", "c", "d")), J.Present("realm_access"), J.Equals(P("cnf", "jkt"), "nope"),
            J.HasWord(P("act", "sub"), "svc-7"), J.HasElement("scope", "openid"), J.Equals(P("realm_access", "roles"), "role-3")]


def directed_requires(J):
    """the directed list's predicate sets as requirements: (path, op, value) either way"""
    return [[J.Require(J.Path(*p), op, val) for p, op, val in reqs] for reqs in MC.PRED_SETS[1:]]


def check_rows(v, toks, e, reqs, rows):
    """err == CheckBatch's == ValidateBatch's; bits == the evaluation on ValidateBatch's map, None for a
    rejected token.  Returns the accepted tokens' bits."""
    full = v.ValidateBatch(toks, e)
    assert [r[1] for r in rows] == v.CheckBatch(toks, e) == [r[1] for r in full]
    out = []
    for (bits, err), (m, _) in zip(rows, full):
        if err is not None:
            assert bits is None
            continue
        assert bits == MC.evaluate(m, reqs), (m, bits, reqs)
        out.append(bits)
    return out


def test_requirements_are_decided_on_the_device(crafted, J):
    v, toks, _ = crafted
    seen = []
    for ex in EXPECTED_SETS[:2]:
        for reqs in [keycloak_requires(J)] + directed_requires(J):
            e = E(J, ex, CC.T0 + 30)
            stats = {}
            rows = v.MatchBatch(toks, reqs, e, stats)
            assert stats == {"scanned": len(toks), "host": 0}      # an entry that defers everything fails here
            seen += check_rows(v, toks, e, reqs, rows)
    assert len(seen) > 100 and len(set(seen)) > 20
    e = E(J, {}, CC.T0 + 30)
    first = v.MatchBatch(toks[:8], keycloak_requires(J), e)
    # bit 0 up: role-3, uma, realm/admin, email, mail, = "openid email", jkt, x5t (null), = svc-7, r5, a/b/c/d,
    # realm_access, jkt = nope, svc-7 as a word, scope as an array, roles as a string
    assert [b for b, _ in first][3] == 0b0000_1100_1110_1011
    assert [b for b, _ in first][7] == 0b0010_1101_1110_1010
    assert v.MatchBatch(toks[:3], [], e) == [(0, None)] * 3


def test_host_path_tokens_mix_with_decided_ones(crafted, J):
    v, plain, hard = crafted
    toks = []
    for k in range(len(plain)):                              # interleaved: both paths inside every merge chunk
        toks += plain[k:k + 1] + hard[k:k + 1]
        if k % 9 == 0:
            toks.append(tamper(plain[k]))
    toks += ["not-a-jwt"]
    reqs = keycloak_requires(J)
    for ex in EXPECTED_SETS[:2]:
        e = E(J, ex, CC.T0 + 30)
        stats = {}
        rows = v.MatchBatch(toks, reqs, e, stats)
        assert stats["scanned"] >= len(plain) and stats["host"] >= len(hard) > 0
        bits = check_rows(v, toks, e, reqs, rows)
        assert any(b & 0b100 for b in bits)                  # realm/admin, written with an escape: from the map
    # a tampered token carries no bits
    e = E(J, {}, CC.T0 + 30)
    bad = v.MatchBatch([tamper(plain[0]), plain[0], "not-a-jwt"], reqs, e)
    assert bad[0][0] is None and bad[0][1] and bad[2][0] is None and bad[1][1] is None and bad[1][0] is not None
    assert v.MatchBatch([], reqs, e) == []


def test_a_list_over_the_scans_caps_still_answers(crafted, J):
    v, plain, hard = crafted
    P = J.Path
    toks = plain[::2] + hard[::3]
    e = E(J, {}, CC.T0 + 30)
    base = {}
    v.CheckBatch(toks, e, base)
    assert base["scanned"] > 0 and base["host"] > 0
    verified = base["scanned"] + base["host"]
    nine = [J.Present(P("n%d" % k)) for k in range(8)] + [J.HasElement(P("realm_access", "roles"), "role-2")]
    for reqs in (nine, [J.Present(P("a", "b", "c", "d", "e")), J.Present(P("a", "b", "c", "d"))],
                 [J.Equals(P("cnf", "jkt"), "v" * 65), J.Present(P("cnf", "jkt"))],
                 [J.HasElement(P("realm_access", "roles"), "rôle"), J.HasElement(P("realm_access", "roles"), "role-2")],
                 [J.HasWord("scope", "openid email"), J.HasWord("scope", "email")],
                 [J.HasWord("scope", ""), J.HasElement(P("realm_access", "roles"), ""), J.Equals("scope", "")],
                 [J.Equals("scope", 'q"'), J.Present("scope")], [J.Present(P("cnf", "")), J.Present("cnf")]):
        stats = {}
        rows = v.MatchBatch(toks, reqs, e, stats)
        assert stats == {"scanned": 0, "host": verified}
        assert len(check_rows(v, toks, e, reqs, rows)) >= 24        # the Keycloak tokens alone: 20 decided, 4 host
    # equal requirements are scanned once: eighteen would not fit, sixteen with repeats do, and stay on the device
    stats = {}
    reqs = keycloak_requires(J)[:12] + keycloak_requires(J)[:4]
    rows = v.MatchBatch(plain, reqs, e, stats)
    assert stats == {"scanned": len(plain), "host": 0}
    bits = check_rows(v, plain, e, reqs, rows)
    assert all(b >> 12 == b & 0xf for b in bits) and any(b >> 12 for b in bits)
    # seventeen requirements have no bit
    with pytest.raises(ValueError):
        v.MatchBatch(plain[:2], keycloak_requires(J) + [J.Present("x")], e)
    with pytest.raises(ValueError):
        v.MatchBlob("\n".join(plain[:2]).encode(), [J.Present("n%d" % k) for k in range(17)], e)
    with pytest.raises(ValueError):
        v.MatchBatch(plain[:2], [J.Equals("a", "a\0b")], e)
    with pytest.raises(ValueError):
        v.MatchBatch(plain[:2], [J.Present(P("a", "a\0b"))], e)
    with pytest.raises(ValueError):
        J.Present(P())
    with pytest.raises(TypeError):
        J.Equals("a", b"b")
    with pytest.raises(TypeError):
        v.MatchBatch(plain[:2], [("a", 4, "")], e)


def masks_of(cols, n):
    assert len(cols["ok"]) == n and len(cols["match"]) == 4 * n
    return list(struct.unpack("<%dI" % n, cols["match"]))


def test_blob_and_each_forms_equal_the_batch_rows(crafted, J):
    v, plain, hard = crafted
    toks = plain + hard + [tamper(t) for t in plain[:10]] + ["not-a-jwt"]
    blob = "\n".join(toks).encode()
    reqs = keycloak_requires(J)
    e = E(J, EXPECTED_SETS[0], CC.T0 + 30)
    stats, bstats = {}, {}
    cols = v.MatchBlob(blob, reqs, e, bstats)
    rows = v.MatchBatch(toks, reqs, e, stats)
    assert sorted(cols) == ["match", "ok"]
    assert cols["ok"] == v.CheckBlob(blob, e)
    assert bstats == stats and stats["host"] > 0 and stats["scanned"] > 0
    assert masks_of(cols, len(toks)) == [b or 0 for b, _ in rows]
    assert list(cols["ok"]) == [int(err is None) for _, err in rows]
    assert 0 < sum(cols["ok"]) < len(toks)
    # an Expected per token: each row is its own Expected's
    es = [E(J, EXPECTED_SETS[0], CC.T0 + 30), E(J, EXPECTED_SETS[1], CC.T0 + 30), E(J, {}, CC.T0 + 7200)]
    which = [i % 3 for i in range(len(toks))]
    estats = {}
    each = v.MatchBatchEach(toks, reqs, es, which, estats)
    alone = [v.MatchBatch(toks, reqs, x) for x in es]
    assert each == [alone[w][i] for i, w in enumerate(which)]
    assert [err for _, err in each] == v.CheckBatchEach(toks, es, which)
    assert estats["scanned"] > 0 and estats["host"] > 0
    ecols = v.MatchBlobEach(blob, reqs, es, array.array("I", which))
    assert masks_of(ecols, len(toks)) == [b or 0 for b, _ in each]
    assert list(ecols["ok"]) == [int(err is None) for _, err in each]

