"""Validator.RegisteredBatch / RegisteredBlob: CheckBatch's verdict plus the
registered claims the GPU scan read (k_claims_extract), against CheckBatch /
ValidateBatch for the errors and against the oracle's jwt.Claims
(oracle.jws._claims_struct) for the values.

Tokens are crafted as tests/test_gpu_check_batch.py crafts them: payloads of the
claims corpus signed with the committed test key (tests/craft.py).
"""
import struct

import pytest

from oracle import jws
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import craft
from tests.test_gpu_check_batch import E, EXPECTED_SETS, KID, SIG_PREFIX, sign_rs256, tamper

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def J():
    from cap_amd import jwt
    return jwt


@pytest.fixture(scope="module")
def crafted(J):
    """(validator, plain tokens, their segments, hard tokens, their segments)"""
    key = craft.keys()[KID]
    ks, err = J.NewStaticKeySet([J.PublicKey.rsa(key.n.to_bytes(key.k, "big"), key.e)])
    assert err is None
    v, _ = J.NewValidator(ks)
    C = CC.corpus()
    plain = sorted({s for s, _ in C.plain})[::2] + sorted({s for s, _, _ in XC.directed()[::97]})
    b64ok = lambda s: s and all(c in CC.B64 for c in s) and len(s) % 4 != 1
    hard = sorted({s for s, _ in C.hard + C.random[:600] if b64ok(s)})[::4]
    assert len(plain) > 100 and len(hard) > 50
    return v, [sign_rs256(s.decode()) for s in plain], plain, [sign_rs256(s.decode()) for s in hard], hard


def oracle_claims(seg):
    return jws._claims_struct(jws._claims_map(XC.payload_of(seg)))[0]


def check_rows(rows, segs, errs):
    """errors equal `errs`; an accepted token's claims are the oracle's, a rejected one has None"""
    assert [r[1] for r in rows] == errs
    n_ok = 0
    for (claims, err), seg in zip(rows, segs):
        if err is not None:
            assert claims is None
            continue
        n_ok += 1
        assert claims == oracle_claims(seg), (XC.payload_of(seg), claims)
    return n_ok


def test_plain_tokens_are_decided_on_the_device_with_the_oracles_claims(crafted, J):
    v, toks, segs, _, _ = crafted
    n_ok = 0
    for ex in EXPECTED_SETS:
        for now_s in (CC.T0 + 30, CC.T0 + 700):
            e = E(J, ex, now_s)
            stats = {}
            rows = v.RegisteredBatch(toks, e, stats)
            assert stats == {"scanned": len(toks), "host": 0}      # an entry that defers everything fails here
            errs = v.CheckBatch(toks, e)
            assert errs == [r[1] for r in v.ValidateBatch(toks, e)]
            n_ok += check_rows(rows, segs, errs)
    assert n_ok > 100
    # every value kind occurred on an accepted row
    rows = v.RegisteredBatch(toks, E(J, {}, CC.T0 + 30))
    got = [c for c, err in rows if err is None]
    assert any(len(c["aud"]) > 1 for c in got) and any(c["aud"] == [] for c in got)
    assert any(c["exp"] is None for c in got) and any(c["exp"] is not None for c in got)
    assert any(c["sub"] for c in got) and any(c["iss"] for c in got) and any(c["jti"] for c in got)


def test_hard_tokens_take_both_paths_and_keep_the_claims(crafted, J):
    v, _, _, toks, segs = crafted
    # an escape or a byte >= 0x80 anywhere in the payload: only the host path can have accepted it
    needs_host = [b"\\" in XC.payload_of(s) or max(XC.payload_of(s), default=0) >= 0x80 for s in segs]
    accepted = []
    for ex in EXPECTED_SETS[:2]:
        e = E(J, ex, CC.T0 + 30)
        stats = {}
        rows = v.RegisteredBatch(toks, e, stats)
        assert stats["host"] > 10 and stats["scanned"] > 10
        errs = v.CheckBatch(toks, e)
        assert errs == [r[1] for r in v.ValidateBatch(toks, e)]
        check_rows(rows, segs, errs)
        accepted += [h for h, err in zip(needs_host, errs) if err is None]
    assert True in accepted and False in accepted           # claims from the host struct and from the records


def test_signature_parse_and_alg_errors_carry_no_claims(crafted, J):
    v, plain, _, _, _ = crafted
    e = E(J, dict(CC.FULL, Issuer="other"), CC.T0 + 30)
    bad = [tamper(t) for t in plain[:40]] + ["not-a-jwt", "a.b"]
    rows = v.RegisteredBatch(bad, e)
    assert all(c is None for c, _ in rows)
    assert [r[1] for r in rows[:40]] == [SIG_PREFIX + "no known key successfully validated the token signature"] * 40
    assert [r[1] for r in rows] == v.CheckBatch(bad, e) == [r[1] for r in v.ValidateBatch(bad, e)]
    for algs in (("ES256",), ("HS256",)):                   # the alg header error, whatever the claims say
        e = E(J, dict(CC.FULL, Issuer="other"), CC.T0 + 30, algs=algs)
        rows = v.RegisteredBatch(plain[:40] + bad[:5], e)
        assert [r[1] for r in rows] == v.CheckBatch(plain[:40] + bad[:5], e)
        assert all(c is None for c, _ in rows)
        assert all(err.startswith("invalid algorithm (alg) header parameter: ") for _, err in rows[:40])
        assert all(err.startswith(SIG_PREFIX) for _, err in rows[40:])
    assert v.RegisteredBatch([], e) == []


def unpack_blob(cols, n):
    """RegisteredBlob's columns -> RegisteredBatch's rows (claims or None per token)"""
    u32 = lambda b: struct.unpack("<%dI" % (len(b) // 4), b)
    i64 = lambda b: struct.unpack("<%dq" % (len(b) // 8), b)
    assert len(cols["ok"]) == n and len(cols["present"]) == n
    dates = {k: i64(cols[k]) for k in ("exp", "nbf", "iat")}
    strs = {}
    for k in ("iss", "sub", "jti"):
        off, data = cols[k]
        off = u32(off)
        assert len(off) == n + 1 and off[0] == 0 and off[-1] == len(data)
        strs[k] = [data[off[i]:off[i + 1]].decode() for i in range(n)]
    tok_off, el_off, data = cols["aud"]
    tok_off, el_off = u32(tok_off), u32(el_off)
    assert len(tok_off) == n + 1 and tok_off[0] == 0 and tok_off[-1] == len(el_off) - 1 and el_off[-1] == len(data)
    rows = []
    for i in range(n):
        aud = [data[el_off[k]:el_off[k + 1]].decode() for k in range(tok_off[i], tok_off[i + 1])]
        row = {k: strs[k][i] for k in strs}
        row["aud"] = aud
        for bit, k in ((5, "exp"), (6, "nbf"), (7, "iat")):
            row[k] = dates[k][i] if (cols["present"][i] >> bit) & 1 else None
            assert row[k] is not None or dates[k][i] == 0
        if not cols["ok"][i]:                               # the rows of a rejected token are empty
            assert row == {"iss": "", "sub": "", "jti": "", "aud": [], "exp": None, "nbf": None, "iat": None}
            row = None
        rows.append(row)
    return rows


def test_blob_columns_equal_the_batch_rows(crafted, J):
    v, plain, _, hard, _ = crafted
    toks = plain + hard + [tamper(t) for t in plain[:20]] + ["not-a-jwt", "a.b"]
    blob = "\n".join(toks).encode()
    for ex in EXPECTED_SETS[:2]:
        e = E(J, ex, CC.T0 + 30)
        stats, bstats = {}, {}
        cols = v.RegisteredBlob(blob, e, bstats)
        rows = v.RegisteredBatch(toks, e, stats)
        assert cols["ok"] == v.CheckBlob(blob, e)
        assert bstats == stats and stats["scanned"] >= len(plain) and stats["host"] > 0
        assert unpack_blob(cols, len(toks)) == [c for c, _ in rows]
        assert 0 < sum(cols["ok"]) < len(toks)
