"""Validator.SelectBatch / SelectBlob / SelectBatchEach with Path elements: the
claims inside objects, read by the GPU scan (k_claims_paths_each), against
ValidateBatch's claims map walked in Python for the values and CheckBatch for
the errors.

Tokens are crafted as tests/test_gpu_select_batch.py crafts them: payloads of
the claims corpus, of the directed list of tests/claims_paths_cases.py and a few
that carry realm_access / cnf objects as Keycloak and DPoP tokens do, signed
with the committed test key (tests/craft.py).  Payloads with an escape take the
host path.
"""
import pytest

from tests import claims_corpus as CC
from tests import claims_paths_cases as PC
from tests import claims_select_cases as SC
from tests import craft
from tests.test_gpu_check_batch import E, EXPECTED_SETS, KID, sign_rs256, tamper
from tests.test_gpu_select_batch import blob_values

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def J():
    from cap_amd import jwt
    return jwt


def keycloak(k, escape=False):
    """an access token's payload with nested role and confirmation claims; escape: one the scan leaves to the host"""
    roles = b'["offline_access","uma_authorization","role-%d"]' % k
    if escape:
        roles = b'["realm\\/admin","role-%d"]' % k
    return (b'{"exp":%d,"iat":%d,"iss":"https://example.com/","aud":"www.example.com","sub":"alice@example.com",'
            b'"jti":"std","realm_access":{"roles":%s},"resource_access":{"app":{"roles":["r%d"]},"account":{"roles":[]}},'
            b'"cnf":{"jkt":"0ZcOCORZNYy-DWpqq30jZyJGHTN0d2HglBV3uiguA4I","x5t#S256":null},"act":{"sub":"svc-%d"},'
            b'"scope":"openid email","a.b":{"c":%d},"a":{"b":{"c":{"d":%d.5}}}}'
            % (CC.T0 + 600, CC.T0, roles, k, k, k, k))


@pytest.fixture(scope="module")
def crafted(J):
    """(validator, tokens the scan decides, tokens it leaves to the host)"""
    key = craft.keys()[KID]
    ks, err = J.NewStaticKeySet([J.PublicKey.rsa(key.n.to_bytes(key.k, "big"), key.e)])
    assert err is None
    v, _ = J.NewValidator(ks)
    C = CC.corpus()
    plain = ([CC.b64(keycloak(k)) for k in range(40)] + sorted({s for s, _, _ in PC.directed()})
             + sorted({s for s, _ in C.plain})[::6])
    hard = [CC.b64(keycloak(k, escape=True)) for k in range(12)]
    return v, [sign_rs256(s.decode()) for s in plain], [sign_rs256(s.decode()) for s in hard]


def paths8(J):
    P = J.Path
    return [P("realm_access", "roles"), "scope", P("resource_access", "app", "roles"), P("cnf", "jkt"), P("cnf", "x5t#S256"),
            P("act", "sub"), P("a", "b", "c", "d"), P("a.b")]


def check_rows(v, toks, e, names, rows):
    """err == CheckBatch's == ValidateBatch's; values == ValidateBatch's map walked
    along each element, keyed by the element as given.  Returns the accepted rows' values."""
    full = v.ValidateBatch(toks, e)
    assert [r[2] for r in rows] == v.CheckBatch(toks, e) == [r[1] for r in full]
    assert [r[0] for r in rows] == [r[0] for r in v.RegisteredBatch(toks, e)]
    out = []
    for (claims, values, err), (m, _) in zip(rows, full):
        if err is not None:
            assert claims is None and values is None
            continue
        want = {}
        for el in names:
            present, val = PC.walk(m, el if isinstance(el, tuple) else (el,))
            if present:
                want[el] = val
        assert SC.same(values, want), (values, want)
        out.append(values)
    return out


def test_paths_are_decided_on_the_device_with_the_maps_values(crafted, J):
    v, toks, _ = crafted
    P = J.Path
    seen = []
    for ex in EXPECTED_SETS[:2]:
        for names in (paths8(J), [P("a", "b"), P("a"), "a"], [P("realm_access", "roles")]):
            e = E(J, ex, CC.T0 + 30)
            stats = {}
            rows = v.SelectBatch(toks, names, e, stats)
            assert stats == {"scanned": len(toks), "host": 0}      # an entry that defers everything fails here
            seen += check_rows(v, toks, e, names, rows)
    assert len(seen) > 100
    first = [vals for vals in seen if P("cnf", "jkt") in vals][0]
    assert first[P("realm_access", "roles")] == ["offline_access", "uma_authorization", "role-0"]
    assert first[P("cnf", "x5t#S256")] is None and first[P("act", "sub")] == "svc-0" and first[P("a", "b", "c", "d")] == 0.5
    assert first[P("a.b")] == {"c": 0.0} and first["scope"] == "openid email"


def test_host_path_tokens_mix_with_decided_ones(crafted, J):
    v, plain, hard = crafted
    toks = []
    for k in range(len(plain)):                              # interleaved: both paths inside every merge chunk
        toks += plain[k:k + 1] + hard[k:k + 1]
        if k % 9 == 0:
            toks.append(tamper(plain[k]))
    toks += ["not-a-jwt"]
    names = paths8(J)
    for ex in EXPECTED_SETS[:2]:
        e = E(J, ex, CC.T0 + 30)
        stats = {}
        rows = v.SelectBatch(toks, names, e, stats)
        assert stats["scanned"] >= len(plain) and stats["host"] >= len(hard) > 0
        vals = check_rows(v, toks, e, names, rows)
        assert any(x.get(J.Path("realm_access", "roles")) == ["realm/admin", "role-3"] for x in vals)     # from the map
    assert v.SelectBatch([], names, E(J, {}, CC.T0 + 30)) == []


def test_a_path_list_the_scan_refuses_still_answers(crafted, J):
    v, plain, hard = crafted
    P = J.Path
    toks = plain[::2] + hard[::3]
    e = E(J, {}, CC.T0 + 30)
    base = {}
    v.RegisteredBatch(toks, e, base)
    verified = base["scanned"] + base["host"]
    nine = paths8(J) + [P("realm_access", "groups")]
    for names in (nine, [P("a", "b", "c", "d", "e")], [P("cnf", "L" * 65)], [P("realm_access", "rôles")],
                  [P("cnf", 'q"')], [P("cnf", "")]):
        stats = {}
        rows = v.SelectBatch(toks, names, e, stats)
        assert stats == {"scanned": 0, "host": verified}
        assert len(check_rows(v, toks, e, names, rows)) >= 24        # the Keycloak tokens alone: 20 decided, 4 host
    # equal paths share a slot: ten elements, eight distinct, still the scan
    stats = {}
    names = paths8(J) + [P("cnf", "jkt"), P("scope")]
    rows = v.SelectBatch(plain, names, e, stats)
    assert stats == {"scanned": len(plain), "host": 0}
    check_rows(v, plain, e, names, rows)
    with pytest.raises(ValueError):
        v.SelectBatch(plain[:2], [P("a", "a\0b")], e)
    with pytest.raises(ValueError):
        P()
    with pytest.raises(TypeError):
        P("a", b"b")


def test_blob_and_each_forms_equal_the_batch_rows(crafted, J):
    v, plain, hard = crafted
    toks = plain + hard + [tamper(t) for t in plain[:10]] + ["not-a-jwt"]
    blob = "\n".join(toks).encode()
    names = paths8(J)
    e = E(J, EXPECTED_SETS[0], CC.T0 + 30)
    stats, bstats = {}, {}
    cols = v.SelectBlob(blob, names, e, bstats)
    rows = v.SelectBatch(toks, names, e, stats)
    assert cols["ok"] == v.CheckBlob(blob, e)
    assert bstats == stats and stats["host"] > 0 and stats["scanned"] > 0
    got = blob_values(cols, names, len(toks))
    assert all((g is None) == (r[1] is None) for g, r in zip(got, rows))
    assert all(SC.same(g, r[1]) for g, r in zip(got, rows) if g is not None)
    assert 0 < sum(cols["ok"]) < len(toks)
    # an Expected per token: each row is its own Expected's
    es = [E(J, EXPECTED_SETS[0], CC.T0 + 30), E(J, EXPECTED_SETS[1], CC.T0 + 30), E(J, {}, CC.T0 + 7200)]
    which = [i % 3 for i in range(len(toks))]
    estats = {}
    each = v.SelectBatchEach(toks, names, es, which, estats)
    alone = [v.SelectBatch(toks, names, x) for x in es]
    assert each == [alone[w][i] for i, w in enumerate(which)]
    assert estats["scanned"] > 0 and estats["host"] > 0
    import array
    ecols = v.SelectBlobEach(blob, names, es, array.array("I", which))
    egot = blob_values(ecols, names, len(toks))
    assert all((g is None) == (r[1] is None) and (g is None or SC.same(g, r[1])) for g, r in zip(egot, each))
    # a list of names alone is today's call: the same rows as before
    assert v.SelectBatch(toks, ["scope", "cnf"], e) == [
        (c, None if x is None else {k[0]: y for k, y in x.items()}, err)
        for c, x, err in v.SelectBatch(toks, [J.Path("scope"), J.Path("cnf")], e)]
