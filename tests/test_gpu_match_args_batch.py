"""Validator.MatchBatchArgs / MatchBlobArgs / MatchBatchArgsEach / MatchBlobArgsEach:
requirements whose other side is the token's own operand (a nonce per token, a
thumbprint for cnf.jkt) or a number (auth_time against a bound per token),
answered by the GPU scan (k_claims_match_args), against ValidateBatch for the
errors and a plain-Python evaluation on ValidateBatch's claims map for the bits.

Tokens are crafted and signed with the committed test key (tests/craft.py): an
ID-token payload with its own nonce, an integer auth_time and a nested cnf.jkt;
a tampered signature, an expired token, payloads the scan leaves to the host (an
escape, a fractional auth_time) and operands the scan refuses.
"""
import array
import struct

import pytest

from tests import claims_corpus as CC
from tests import claims_match_args_cases as AC
from tests import craft
from tests.test_gpu_check_batch import E, EXPECTED_SETS, KID, sign_rs256, tamper

pytestmark = pytest.mark.gpu
JKT = "0ZcOCORZNYy-DWpqq30jZyJGHTN0d2HglBV3uiguA4I"


@pytest.fixture(scope="module")
def J():
    from cap_amd import jwt
    return jwt


def nonce_of(k):
    return "n-%02d_WzA2Mj%08x" % (k % 100, k * 2654435761 % (1 << 32))       # distinct


def id_token(k, kind="plain"):
    auth = b"%d" % (CC.T0 - 10 * k)
    exp = CC.T0 + 600
    nonce = nonce_of(k).encode()
    if kind == "escape":
        nonce = nonce[:5] + b"\\u002f" + nonce[5:]                  # the claim holds a "/" the text spells with an escape
    if kind == "fraction":
        auth += b".5"
    if kind == "expired":
        exp = CC.T0 - 600
    return (b'{"iss":"https://example.com/","aud":"www.example.com","sub":"alice@example.com","jti":"std","exp":%d,"iat":%d,'
            b'"nonce":"%s","auth_time":%s,"cnf":{"jkt":"%s%d"},"acr":"%d"}' % (exp, CC.T0, nonce, auth, JKT.encode(), k % 3, k % 2))


def truth(k, kind):
    """the operands that make every requirement of REQS hold for id_token(k, kind)"""
    n = nonce_of(k)
    if kind == "escape":
        n = n[:5] + "/" + n[5:]
    return n, JKT + "%d" % (k % 3), CC.T0 - 10 * k


@pytest.fixture(scope="module")
def crafted(J):
    """(validator, tokens, kinds, operand columns): every sixth token's operands are off by something"""
    key = craft.keys()[KID]
    ks, err = J.NewStaticKeySet([J.PublicKey.rsa(key.n.to_bytes(key.k, "big"), key.e)])
    assert err is None
    v, _ = J.NewValidator(ks)
    kinds = ["plain"] * 48 + ["escape"] * 6 + ["fraction"] * 6 + ["expired"] * 3 + ["tampered"] * 3
    kinds = [kinds[(7 * k) % len(kinds)] for k in range(len(kinds))]           # interleaved
    toks, nonces, jkts, bounds = [], [], [], []
    for k, kind in enumerate(kinds):
        t = sign_rs256(CC.b64(id_token(k, "plain" if kind == "tampered" else kind)).decode())
        toks.append(tamper(t) if kind == "tampered" else t)
        n, j, a = truth(k, kind)
        m = k % 6
        nonces.append(n if m != 1 else AC.flip(n.encode(), len(n) - 1).decode())
        jkts.append(j if m != 2 else j[:-1])
        bounds.append(a if m != 3 else a + 1)
    return v, toks, kinds, [nonces, jkts], [bounds]


def requires(J):
    P = J.Path
    return [J.EqualsEach("nonce", 0), J.AtLeastEach("auth_time", 0), J.EqualsEach(P("cnf", "jkt"), 1), J.AtMostEach("auth_time", 0),
            J.AtLeast("auth_time", CC.T0 - 300), J.AtMost("auth_time", CC.T0), J.Equals("acr", "1"), J.Present(P("cnf", "jkt")),
            J.Equals("aud", "www.example.com"), J.EqualsEach("sub", 1)]


def plain_requires(reqs):
    """J's requirements as (path, op, value) of tests/claims_match_args_cases.py"""
    out = []
    for r in reqs:
        path, op = tuple(r[0]), r[1]
        out.append((path, op, r[2] if op <= AC.PRESENT else r[3] if op in (AC.NUM_GE, AC.NUM_LE) else r[4]))
    return out


def check_rows(v, toks, e, reqs, strs, nums, rows):
    """err == ValidateBatch's == CheckBatch's; bits == the evaluation on ValidateBatch's map with the token's operands"""
    full = v.ValidateBatch(toks, e)
    assert [r[1] for r in rows] == v.CheckBatch(toks, e) == [r[1] for r in full]
    pr = plain_requires(reqs)
    out = []
    for i, ((bits, err), (m, _)) in enumerate(zip(rows, full)):
        if err is not None:
            assert bits is None
            continue
        s = [c[i].encode() if isinstance(c[i], str) else bytes(c[i]) for c in strs]
        assert bits == AC.evaluate(m, pr, s, [c[i] for c in nums]), (i, m, bits)
        out.append(bits)
    return out


def test_operands_are_compared_on_the_device(crafted, J):
    v, toks, kinds, strs, nums = crafted
    reqs = requires(J)
    host_kinds = sum(k in ("escape", "fraction") for k in kinds)
    verified = sum(k != "tampered" for k in kinds)
    for ex in EXPECTED_SETS[:2]:
        e = E(J, ex, CC.T0 + 30)
        stats = {}
        rows = v.MatchBatchArgs(toks, reqs, strs, nums, e, stats)
        assert stats == {"scanned": verified - host_kinds, "host": host_kinds}      # the decided tokens were scanned
        bits = check_rows(v, toks, e, reqs, strs, nums, rows)
        # bit 0 up: nonce, auth_time >= n, jkt, auth_time <= n, >= T0 - 300, <= T0, acr = 1, jkt present, aud, sub = jkt
        assert len(bits) == 60 and sum(b & 0b1111 == 0b1111 for b in bits) >= 25
        assert all(sum(not (b >> k) & 1 for b in bits) >= 5 for k in (0, 1, 2))       # each operand fails somewhere
        assert all(b & 0b1110000000 == 0b0110000000 for b in bits)
    for i, kind in enumerate(kinds):
        assert (rows[i][1] is None) == (kind not in ("expired", "tampered")), (i, kind, rows[i])
    # a list without a numeric requirement leaves the fractional tokens to the device
    stats = {}
    e = E(J, {}, CC.T0 + 30)
    rows = v.MatchBatchArgs(toks, [reqs[0], reqs[2], reqs[9]], strs, [], e, stats)
    assert stats == {"scanned": verified - kinds.count("escape"), "host": kinds.count("escape")}
    check_rows(v, toks, e, [reqs[0], reqs[2], reqs[9]], strs, [], rows)
    # number columns as an array and as a list of int; string columns as bytes give the same rows
    want = v.MatchBatchArgs(toks, reqs, strs, nums, e)
    assert v.MatchBatchArgs(toks, reqs, strs, [array.array("q", nums[0])], e) == want
    assert v.MatchBatchArgs(toks, reqs, [[s.encode() for s in c] for c in strs], nums, e) == want
    assert v.MatchBatchArgs([], reqs, [[], []], [[]], e) == []
    assert v.MatchBatchArgs(toks[:3], [], expected=e) == [(0, None)] * 3


def test_a_refused_operand_and_lists_over_the_caps_take_the_host_path(crafted, J):
    v, toks, kinds, strs, nums = crafted
    reqs = requires(J)
    e = E(J, {}, CC.T0 + 30)
    base = {}
    want = v.MatchBatchArgs(toks, reqs, strs, nums, e, base)
    # operands the scan refuses: those tokens alone move to the host path, every row stays what it was
    bad = [list(c) for c in strs]
    moved = [i for i, k in enumerate(kinds) if k == "plain"][:4]
    bad[0][moved[0]] = "nønce"
    bad[1][moved[1]] = "v" * 65
    bad[0][moved[2]] = 'say "hi"'
    bad[1][moved[3]] = "tab\there"
    stats = {}
    rows = v.MatchBatchArgs(toks, reqs, bad, nums, e, stats)
    assert stats == {"scanned": base["scanned"] - 4, "host": base["host"] + 4}
    check_rows(v, toks, e, reqs, bad, nums, rows)
    assert [r for i, r in enumerate(rows) if i not in moved] == [r for i, r in enumerate(want) if i not in moved]
    # an operand with bytes >= 0x80 that equals the claim: the host path compares the bytes
    payload = ('{"exp":%d,"iat":%d,"nonce":"nønce","auth_time":5}' % (CC.T0 + 600, CC.T0)).encode()
    odd = sign_rs256(CC.b64(payload).decode())
    stats = {}
    assert v.MatchBatchArgs([odd, odd], [J.EqualsEach("nonce", 0), J.AtMostEach("auth_time", 0)], [["nønce", "nonce"]], [[5, 4]],
                            e, stats) == [(0b11, None), (0, None)]
    assert stats == {"scanned": 1, "host": 1}
    # lists over the caps: five columns of a kind, nine paths
    verified = base["scanned"] + base["host"]
    five = strs + [strs[0]] * 3
    over = reqs + [J.EqualsEach("nonce", 4)]
    stats = {}
    rows = v.MatchBatchArgs(toks, over, five, nums, e, stats)
    assert stats == {"scanned": 0, "host": verified}
    assert [(b and b & 0x3ff, err) for b, err in rows] == want
    assert all(b >> 10 == b & 1 for b, err in rows if err is None)
    nine = reqs[:8] + [J.Present("p%d" % k) for k in range(5)]
    stats = {}
    rows = v.MatchBatchArgs(toks, nine, strs, nums, e, stats)
    assert stats == {"scanned": 0, "host": verified}
    check_rows(v, toks, e, nine, strs, nums, rows)
    # what no path takes
    for call in (lambda: v.MatchBatchArgs(toks, reqs, [strs[0][:-1], strs[1]], nums, e),
                 lambda: v.MatchBatchArgs(toks, reqs, strs, [nums[0][:-1]], e),
                 lambda: v.MatchBatchArgs(toks, reqs, strs[:1], nums, e),
                 lambda: v.MatchBatchArgs(toks, reqs, strs, [], e),
                 lambda: v.MatchBatchArgs(toks, reqs + [J.AtLeast("n%d" % k, k) for k in range(7)], strs, nums, e),
                 lambda: v.MatchBatchArgs(toks[:1], reqs, [["a\0b"], ["x"]], [[1]], e),
                 lambda: v.MatchBatchArgs(toks[:1], reqs, [["a"], ["x"]], [[1 << 63]], e),
                 lambda: v.MatchBlobArgs("\n".join(toks).encode(), reqs, [b"only-one"], nums, e)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        J.AtLeast("a", 1.5)
    with pytest.raises(TypeError):
        v.MatchBatch(toks[:1], [J.AtLeast("a", 1)], e)                  # the MatchBatch family takes its own four alone


def masks_of(cols, n):
    assert len(cols["ok"]) == n and len(cols["match"]) == 4 * n
    return list(struct.unpack("<%dI" % n, cols["match"]))


def test_blob_and_each_forms_equal_the_batch_rows(crafted, J):
    v, toks, kinds, strs, nums = crafted
    toks = toks + ["not-a-jwt"]
    strs = [c + [""] for c in strs]
    nums = [c + [0] for c in nums]
    blob = "\n".join(toks).encode()
    scols = [("\n".join(c) + "\n").encode() for c in strs]
    assert scols[0].endswith(b"\n\n")                                   # the last operand is "": an empty line
    reqs = requires(J)
    e = E(J, EXPECTED_SETS[0], CC.T0 + 30)
    stats, bstats = {}, {}
    cols = v.MatchBlobArgs(blob, reqs, scols, [array.array("q", nums[0])], e, bstats)
    rows = v.MatchBatchArgs(toks, reqs, strs, nums, e, stats)
    assert sorted(cols) == ["match", "ok"]
    assert cols["ok"] == v.CheckBlob(blob, e)
    assert bstats == stats and stats["host"] > 0 and stats["scanned"] > 0
    assert masks_of(cols, len(toks)) == [b or 0 for b, _ in rows]
    assert list(cols["ok"]) == [int(err is None) for _, err in rows]
    assert 0 < sum(cols["ok"]) < len(toks) and len(set(masks_of(cols, len(toks)))) > 6
    assert v.MatchBlobArgs(blob, reqs, ["\n".join(c).encode() for c in strs], nums, e) == cols    # without the last newline
    # an Expected per token: each row is its own Expected's
    es = [E(J, EXPECTED_SETS[0], CC.T0 + 30), E(J, EXPECTED_SETS[1], CC.T0 + 30), E(J, {}, CC.T0 + 7200)]
    which = [i % 3 for i in range(len(toks))]
    estats = {}
    each = v.MatchBatchArgsEach(toks, reqs, es, which, strs, nums, estats)
    alone = [v.MatchBatchArgs(toks, reqs, strs, nums, x) for x in es]
    assert each == [alone[w][i] for i, w in enumerate(which)]
    assert [err for _, err in each] == v.CheckBatchEach(toks, es, which)
    assert estats["scanned"] > 0 and estats["host"] > 0
    ecols = v.MatchBlobArgsEach(blob, reqs, es, array.array("I", which), scols, nums)
    assert masks_of(ecols, len(toks)) == [b or 0 for b, _ in each]
    assert list(ecols["ok"]) == [int(err is None) for _, err in each]
