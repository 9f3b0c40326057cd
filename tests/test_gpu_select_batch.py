"""Validator.SelectBatch / SelectBlob: RegisteredBatch's verdict and claims plus
the top-level claims the caller names, read by the GPU scan (k_claims_select),
against CheckBatch / ValidateBatch for the errors, RegisteredBatch for the
claims and ValidateBatch's claims map for the values.

Tokens are crafted as tests/test_gpu_check_batch.py crafts them: payloads of the
claims corpus and of the directed list of tests/claims_select_cases.py, signed
with the committed test key (tests/craft.py).
"""
import json
import struct

import pytest

from tests import claims_corpus as CC
from tests import claims_select_cases as SC
from tests import craft
from tests.test_gpu_check_batch import E, EXPECTED_SETS, KID, SIG_PREFIX, sign_rs256, tamper
from tests.test_gpu_registered_batch import unpack_blob

pytestmark = pytest.mark.gpu

# keys of the directed payloads and of the corpus: a set of 8 and a small one
NAMES8 = ["scope", "x", "name", "deep", "aud", "a", "b", "sub"]
NAMES2 = ["scope", "roles"]
NINE = NAMES8 + ["tenant"]


@pytest.fixture(scope="module")
def J():
    from cap_amd import jwt
    return jwt


@pytest.fixture(scope="module")
def crafted(J):
    """(validator, plain tokens, hard tokens)"""
    key = craft.keys()[KID]
    ks, err = J.NewStaticKeySet([J.PublicKey.rsa(key.n.to_bytes(key.k, "big"), key.e)])
    assert err is None
    v, _ = J.NewValidator(ks)
    C = CC.corpus()
    plain = sorted({s for s, _ in C.plain})[::3] + sorted({s for s, _, _ in SC.directed()})
    b64ok = lambda s: s and all(c in CC.B64 for c in s) and len(s) % 4 != 1
    hard = sorted({s for s, _ in C.hard + C.random[:600] if b64ok(s)})[::4] + [SC.host_only()[0][0]]
    assert len(plain) > 300 and len(hard) > 50
    return v, [sign_rs256(s.decode()) for s in plain], [sign_rs256(s.decode()) for s in hard]


def check_rows(v, toks, e, names, rows):
    """err == CheckBatch's == ValidateBatch's; claims == RegisteredBatch's; values ==
    ValidateBatch's map entries under the names (floats by their 8 bytes).
    Returns the accepted rows' values."""
    full = v.ValidateBatch(toks, e)
    errs = v.CheckBatch(toks, e)
    assert errs == [r[1] for r in full]
    assert [r[2] for r in rows] == errs
    assert [r[0] for r in rows] == [r[0] for r in v.RegisteredBatch(toks, e)]
    out = []
    for (claims, values, err), (m, _) in zip(rows, full):
        if err is not None:
            assert claims is None and values is None
            continue
        want = {k: m[k] for k in names if k in m}
        assert SC.same(values, want), (values, want)
        out.append(values)
    return out


def test_plain_tokens_are_decided_on_the_device_with_the_maps_values(crafted, J):
    v, toks, _ = crafted
    seen = []
    for ex in EXPECTED_SETS[:2]:
        for names in (NAMES8, NAMES2, []):
            e = E(J, ex, CC.T0 + 30)
            stats = {}
            rows = v.SelectBatch(toks, names, e, stats)
            assert stats == {"scanned": len(toks), "host": 0}      # an entry that defers everything fails here
            seen += check_rows(v, toks, e, names, rows)
    assert len(seen) > 100
    # every value kind occurred on an accepted row, -0 and a non-ASCII string among them
    kinds = {type(x) for vals in seen for x in vals.values()}
    assert kinds == {str, float, bool, type(None), list, dict}
    assert any(struct.pack("<d", x) == struct.pack("<d", -0.0) for vals in seen for x in vals.values()
               if isinstance(x, float))
    assert any(isinstance(x, str) and not x.isascii() for vals in seen for x in vals.values())
    assert any(len(vals) == 0 for vals in seen) and any(len(vals) >= 3 for vals in seen)


def test_hard_and_tampered_tokens_mix_with_decided_ones(crafted, J):
    v, plain, hard = crafted
    toks = []
    for k in range(max(len(plain), len(hard))):              # interleaved: both paths inside every merge chunk
        toks += plain[k:k + 1] + hard[k:k + 1]
        if k % 7 == 0:
            toks.append(tamper(plain[k % len(plain)]))
    toks += ["not-a-jwt", "a.b"]
    accepted = 0
    for ex in EXPECTED_SETS[:2]:
        e = E(J, ex, CC.T0 + 30)
        stats = {}
        rows = v.SelectBatch(toks, NAMES8, e, stats)
        assert stats["scanned"] >= len(plain) and stats["host"] > 10
        accepted += len(check_rows(v, toks, e, NAMES8, rows))
        assert sum(1 for r in rows if r[2] and r[2].startswith(SIG_PREFIX)) > len(plain) // 7
    assert accepted > 50                                     # few pass the full Expected, many the empty one
    for algs in (("ES256",),):                               # the alg header error, whatever the claims say
        e = E(J, {}, CC.T0 + 30, algs=algs)
        rows = v.SelectBatch(plain[:40], NAMES2, e)
        assert all(r[0] is None and r[1] is None for r in rows)
        assert [r[2] for r in rows] == v.CheckBatch(plain[:40], e)
    assert v.SelectBatch([], NAMES2, E(J, {}, CC.T0 + 30)) == []


def test_a_name_list_the_scan_refuses_still_answers(crafted, J):
    v, plain, hard = crafted
    toks = plain[::2] + hard[::3]
    e = E(J, {}, CC.T0 + 30)
    base = {}
    v.RegisteredBatch(toks, e, base)
    verified = base["scanned"] + base["host"]
    for names in (NINE, ["scope", "L" * 65], ["scope", "né"], ["scope", 'q"'], ["scope", ""]):
        stats = {}
        rows = v.SelectBatch(toks, names, e, stats)
        assert stats == {"scanned": 0, "host": verified}
        assert len(check_rows(v, toks, e, names, rows)) > 50
    # equal names share a slot: ten names, eight distinct, still the scan
    stats = {}
    names = NAMES8 + ["scope", "sub"]
    rows = v.SelectBatch(plain, names, e, stats)
    assert stats == {"scanned": len(plain), "host": 0}
    check_rows(v, plain, e, names, rows)
    with pytest.raises(ValueError):
        v.SelectBatch(plain[:2], ["a\0b"], e)


def blob_values(cols, names, n):
    """SelectBlob's "sel" columns -> SelectBatch's values dicts (None for a rejected token)"""
    out = [dict() if cols["ok"][i] else None for i in range(n)]
    assert len(cols["sel"]) == len(names)
    for name, c in zip(names, cols["sel"]):
        off = struct.unpack("<%dI" % (n + 1), c["text_off"])
        num = struct.unpack("<%dd" % n, c["num"])
        assert len(c["type"]) == n and off[0] == 0 and off[-1] == len(c["text"])
        for i in range(n):
            t, text = c["type"][i], c["text"][off[i]:off[i + 1]]
            if t not in (1, 2, 7, 8):
                assert text == b""
            if t != 3:
                assert num[i] == 0.0
            if t == 0:
                continue
            assert out[i] is not None, "a rejected token's rows are empty"
            out[i][name] = (text.decode() if t in (1, 2) else num[i] if t == 3 else True if t == 4 else False if t == 5
                            else None if t == 6 else json.loads(text.decode(), parse_int=float))
    return out


def test_blob_columns_equal_the_batch_rows(crafted, J):
    v, plain, hard = crafted
    toks = plain + hard + [tamper(t) for t in plain[:20]] + ["not-a-jwt", "a.b"]
    blob = "\n".join(toks).encode()
    for ex, names in ((EXPECTED_SETS[0], NAMES8), (EXPECTED_SETS[1], NAMES2), (EXPECTED_SETS[0], NINE)):
        e = E(J, ex, CC.T0 + 30)
        stats, bstats = {}, {}
        cols = v.SelectBlob(blob, names, e, bstats)
        rows = v.SelectBatch(toks, names, e, stats)
        assert cols["ok"] == v.CheckBlob(blob, e)
        assert bstats == stats and stats["host"] > 0
        assert (stats["scanned"] == 0) == (names is NINE)
        assert unpack_blob(cols, len(toks)) == [r[0] for r in rows]
        got = blob_values(cols, names, len(toks))
        assert all((g is None) == (r[1] is None) for g, r in zip(got, rows))
        assert all(SC.same(g, r[1]) for g, r in zip(got, rows) if g is not None), [
            (g, r[1]) for g, r in zip(got, rows) if g is not None and not SC.same(g, r[1])][:3]
        assert 0 < sum(cols["ok"]) < len(toks)
        # the columns themselves do not depend on which path decided, but for a string's type byte
        if names is NAMES8:
            other = v.SelectBlob(blob, names + ["tenant"], e)
            for a, b in zip(cols["sel"], other["sel"]):
                assert a["text"] == b["text"] and a["text_off"] == b["text_off"] and a["num"] == b["num"]
                assert bytes(1 if t == 2 else t for t in a["type"]) == b["type"]
