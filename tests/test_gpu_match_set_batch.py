"""Validator.MatchBatchArgs / MatchBlobArgs and their *Each forms with InSet and
AnyElementIn on ClaimSets: is jti on the deny-list, is a group one of the groups
served, answered by the scan (k_claims_match_set) against sets resident on the
device, beside the request's own nonce.

Tokens are crafted and signed with the committed test keys (tests/craft.py,
RS256).  ok / err are ValidateBatch's, and every bit is the plain-Python
evaluation on the claims map ValidateBatch returns.  An escape in a payload goes
through the host path; a tampered token comes back without bits; a host-only set
and five sets give the same rows from the host path; Replace and Close act on
the next call.
"""
import array
import json
import struct

import pytest

from tests import claims_corpus as CC
from tests import craft
from tests.test_gpu_check_batch import KID, b64u, tamper

pytestmark = pytest.mark.gpu
KINDS = ["revoked"] * 5 + ["clean"] * 6 + ["empty", "long", "number", "null", "absent", "groups-string", "groups-nested", "utf8",
                                           "escape", "escape-group", "expired", "tampered", "twice"]
LONG = "L" * 255
REVOKED = ["jti-%d" % k for k in range(0, 200, 2)] + ["", LONG, "jti-0"]
GROUPS = ["admin", "ops", "tenant-7"]


@pytest.fixture(scope="module")
def J():
    from cap_amd import jwt
    return jwt


def sign(payload: bytes) -> str:
    hdr = b64u(json.dumps({"alg": "RS256", "kid": KID}, separators=(",", ":")).encode())
    si = (hdr + "." + CC.b64(payload).decode()).encode()
    key = craft.keys()[KID]
    return si.decode() + "." + b64u(craft.sign_raw(key, craft.pkcs1_em(key.k, 256, si)))


@pytest.fixture(scope="module")
def crafted(J):
    """(validator, tokens, kinds, nonces)"""
    key = craft.keys()[KID]
    ks, err = J.NewStaticKeySet([J.PublicKey.rsa(key.n.to_bytes(key.k, "big"), key.e)])
    assert err is None
    v, _ = J.NewValidator(ks)
    kinds = [KINDS[(5 * k) % len(KINDS)] for k in range(len(KINDS))]             # interleaved
    toks, nonces = [], []
    for k, kind in enumerate(kinds):
        claims = {"iss": "https://example.com/", "aud": "www.example.com", "sub": "alice@example.com", "iat": CC.T0,
                  "exp": CC.T0 + (-600 if kind == "expired" else 600), "nonce": "n-%d" % k,
                  "sid": "jti-%d" % (2 * k if kind in ("revoked", "expired", "tampered", "escape") else 2 * k + 1),
                  "groups": ["g-%d" % k, "ops" if k % 2 else "nobody", {"admin": "admin"}, 7]}
        if kind in ("empty", "long", "utf8"):
            claims["sid"] = {"empty": "", "long": LONG, "utf8": "jti-é"}[kind]
        elif kind in ("number", "null"):
            claims["sid"] = {"number": 4, "null": None}[kind]
        elif kind == "absent":
            del claims["sid"]
        elif kind == "groups-string":
            claims["groups"] = "admin"
        elif kind == "groups-nested":
            claims["groups"] = [["admin"], {"g": "ops"}, "x"]
        payload = json.dumps(claims, separators=(",", ":"), ensure_ascii=False).encode()
        if kind == "escape":
            payload = payload.replace(b'"sid":"jti-', b'"sid":"jti\\u002d')
        elif kind == "escape-group":
            payload = payload.replace(b'"g-%d"' % k, b'"ad\\u006din"')
        elif kind == "twice":
            payload = payload[:-1] + b',"sid":"jti-0","sid":"jti-1"}'            # the last member wins: not revoked
        t = sign(payload)
        toks.append(tamper(t) if kind == "tampered" else t)
        nonces.append("n-%d" % (k if k % 7 else k + 1))
    return v, toks, kinds, nonces


def expected(J, now_s=CC.T0 + 30):
    return J.Expected(Now=lambda: now_s, SigningAlgorithms=["RS256"], Issuer="https://example.com/")


def requires(J, revoked, groups):
    return [J.InSet("sid", revoked), J.AnyElementIn("groups", groups), J.InSet("groups", groups), J.EqualsEach("nonce", 0),
            J.IsString("sid"), J.AnyElementIn("sid", revoked)]


def evaluate(claims, nonce, revoked, groups):
    """The six requirements on a claims map, as Go code on it decides them"""
    sid, grp = claims.get("sid"), claims.get("groups")
    elem = lambda v, s: isinstance(v, list) and any(isinstance(e, str) and e in s for e in v)
    return (int(isinstance(sid, str) and sid in revoked) | int(elem(grp, groups)) << 1 | int(isinstance(grp, str) and grp in groups) << 2 |
            int(claims.get("nonce") == nonce) << 3 | int(isinstance(sid, str)) << 4 | int(elem(sid, revoked)) << 5)


def check_rows(v, crafted, rows, e, revoked=REVOKED, groups=GROUPS):
    _, toks, kinds, nonces = crafted
    full = v.ValidateBatch(toks, e)
    assert [r[1] for r in rows] == [r[1] for r in full] == v.CheckBatch(toks, e)
    for i, ((bits, err), kind) in enumerate(zip(rows, kinds)):
        assert (err is None) == (kind not in ("expired", "tampered")), (i, kind, err)
        if err is not None:
            assert bits is None                                                  # a rejected token carries no bits
            continue
        assert bits == evaluate(full[i][0], nonces[i], set(revoked), set(groups)), (i, kind, bin(bits), full[i][0])
    return [b for b, _ in rows]


def test_sets_are_asked_on_the_device(crafted, J):
    v, toks, kinds, nonces = crafted
    revoked, groups = v.NewClaimSet(REVOKED, seed=11), v.NewClaimSet(GROUPS)
    assert len(revoked) == len(set(REVOKED)) and revoked.info()["seed"] == 11 and not revoked.info()["host_only"]
    assert revoked.info()["nslots"] == 256 and revoked.info()["maxprobe"] >= 1 and groups.info()["n"] == 3
    reqs, e = requires(J, revoked, groups), expected(J)
    stats = {}
    rows = v.MatchBatchArgs(toks, reqs, [nonces], [], e, stats)
    verified = sum(k != "tampered" for k in kinds)
    host = sum(k in ("escape", "escape-group") for k in kinds)
    assert stats == {"scanned": verified - host, "host": host}                   # everything else was decided on the device
    bits = check_rows(v, crafted, rows, e)
    for i, kind in enumerate(kinds):
        if kind in ("revoked", "empty", "long", "escape"):
            assert bits[i] & 0b10001 == 0b10001, (i, kind, bits[i])
        if kind in ("clean", "utf8", "twice", "escape-group"):
            assert bits[i] & 0b10001 == 0b10000, (i, kind, bits[i])
        if kind in ("number", "null", "absent"):
            assert bits[i] & 0b110001 == 0, (i, kind, bits[i])
        if kind == "groups-string":
            assert bits[i] & 0b110 == 0b100
        if kind == "groups-nested":
            assert bits[i] & 0b110 == 0
        if kind == "escape-group":
            assert bits[i] & 0b10 == 0b10                                        # "admin" is admin, on the host path
    assert sum(b is not None and b & 2 == 2 for b in bits) >= 8 and all(b is None or not b & 32 for b in bits)
    assert "InSet" in repr(reqs[0]) and "AnyElementIn" in repr(reqs[1])
    assert v.MatchBatchArgs([], reqs, [[]], [], e) == []
    # the set requirements alone, and beside a hash column
    only = v.MatchBatchArgs(toks, reqs[:2], expected=e)
    assert [b for b, _ in only] == [None if b is None else b & 3 for b in bits]
    withh = v.MatchBatchArgs(toks, reqs + [J.HashOfEach("at_hash", 0)], [nonces], [], e, hashes=[[b"tok"] * len(toks)])
    assert withh == rows                                                         # no at_hash anywhere: the seventh bit never holds


def test_host_only_sets_five_sets_and_what_throws(crafted, J):
    v, toks, kinds, nonces = crafted
    revoked, groups = v.NewClaimSet(REVOKED), v.NewClaimSet(GROUPS)
    e = expected(J)
    want = v.MatchBatchArgs(toks, requires(J, revoked, groups), [nonces], [], e)
    verified = sum(k != "tampered" for k in kinds)
    # a member the device refuses: the set is host-only, every token takes the host path, the rows are the same
    for extra in ("jti-é-other", "x" * 256, 'q"q', "tab\there"):
        ho = v.NewClaimSet(REVOKED + [extra])
        assert ho.info()["host_only"] and ho.info()["nslots"] == 0 and len(ho) == len(set(REVOKED)) + 1
        stats = {}
        assert v.MatchBatchArgs(toks, requires(J, ho, groups), [nonces], [], e, stats) == want
        assert stats == {"scanned": 0, "host": verified}
        ho.Close()
    # ... and one that a payload holds: the host path finds it
    ho = v.NewClaimSet(REVOKED + ["jti-é"])
    rows = v.MatchBatchArgs(toks, requires(J, ho, groups), [nonces], [], e)
    check_rows(v, crafted, rows, e, revoked=REVOKED + ["jti-é"])
    assert [b for b, _ in rows] != [b for b, _ in want]
    ho.Close()
    # five sets: results never depend on the caps
    five = [v.NewClaimSet(REVOKED, seed=k) for k in range(5)]
    for count, scanned in ((3, True), (4, False)):                            # with `groups`: four sets, and five
        reqs = [J.InSet("sid", s) for s in five[:count]] + [J.AnyElementIn("groups", groups)]
        stats = {}
        rows = v.MatchBatchArgs(toks, reqs, [nonces], [], e, stats)
        assert (stats["scanned"] > 0) == scanned and stats["scanned"] + stats["host"] == verified
        for (b, err), (w, werr) in zip(rows, want):
            assert err == werr and (b is None) == (w is None)
            if b is not None:
                assert b == ((1 << count) - 1) * (w & 1) | ((w >> 1) & 1) << count
    for s in five:
        s.Close()
    with pytest.raises(ValueError):
        v.NewClaimSet(["ok", "nul\0"])
    with pytest.raises(ValueError):
        revoked.Replace(["nul\0"])
    with pytest.raises(TypeError):
        v.MatchBatch(toks[:1], [J.InSet("sid", revoked)], e)                    # the MatchBatch family takes its own four alone
    other_ks, _ = J.NewStaticKeySet([J.PublicKey.rsa(craft.keys()[KID].n.to_bytes(craft.keys()[KID].k, "big"), craft.keys()[KID].e)])
    v2, _ = J.NewValidator(other_ks)
    with pytest.raises(ValueError):
        v2.MatchBatchArgs(toks, [J.InSet("sid", revoked)], [], [], e)           # a set of another key set
    # sixteen live sets; the seventeenth raises until one is closed
    more = []
    with pytest.raises(RuntimeError):
        for _ in range(17):
            more.append(v.NewClaimSet(["m"]))
    assert len(more) == 14                                                       # revoked and groups are live too
    more.pop().Close()
    more.append(v.NewClaimSet(["m"]))
    for s in more:
        s.Close()
    assert v.MatchBatchArgs(toks, requires(J, revoked, groups), [nonces], [], e) == want


def test_replace_and_close_act_on_the_next_call(crafted, J):
    v, toks, kinds, nonces = crafted
    revoked, groups = v.NewClaimSet(REVOKED), v.NewClaimSet(GROUPS)
    e = expected(J)
    reqs = requires(J, revoked, groups)
    before = v.MatchBatchArgs(toks, reqs, [nonces], [], e)
    g0 = revoked.info()["generation"]
    odd = ["jti-%d" % k for k in range(1, 200, 2)]
    revoked.Replace(odd)
    assert revoked.info()["generation"] > g0 and len(revoked) == 100
    after = v.MatchBatchArgs(toks, reqs, [nonces], [], e)
    check_rows(v, crafted, after, e, revoked=odd)
    flipped = [i for i, ((a, _), (b, _)) in enumerate(zip(before, after)) if a is not None and (a ^ b) & 1]
    assert len(flipped) >= 12 and all((a is None) == (b is None) and (a is None or (a ^ b) & ~1 == 0) for (a, _), (b, _) in zip(before, after))
    revoked.Replace(REVOKED + ["jti-é"])                                    # to a host-only set, and back
    assert revoked.info()["host_only"]
    check_rows(v, crafted, v.MatchBatchArgs(toks, reqs, [nonces], [], e), e, revoked=REVOKED + ["jti-é"])
    revoked.Replace(REVOKED)
    assert not revoked.info()["host_only"] and v.MatchBatchArgs(toks, reqs, [nonces], [], e) == before
    groups.Close()
    with pytest.raises(ValueError):
        v.MatchBatchArgs(toks, reqs, [nonces], [], e)
    assert v.MatchBatchArgs(toks, [reqs[0], reqs[3]], [nonces], [], e) == [(None if b is None else (b & 1) | (b >> 3 & 1) << 1, err) for b, err in before]


def masks_of(cols, n):
    assert len(cols["ok"]) == n and len(cols["match"]) == 4 * n
    return list(struct.unpack("<%dI" % n, cols["match"]))


def test_blob_and_each_forms_equal_the_batch_rows(crafted, J):
    v, toks, kinds, nonces = crafted
    toks, nonces = toks + ["not-a-jwt"], nonces + [""]
    blob = "\n".join(toks).encode()
    revoked, groups = v.NewClaimSet(REVOKED), v.NewClaimSet(GROUPS)
    reqs, e = requires(J, revoked, groups), expected(J)
    stats, bstats = {}, {}
    rows = v.MatchBatchArgs(toks, reqs, [nonces], [], e, stats)
    cols = v.MatchBlobArgs(blob, reqs, ["\n".join(nonces).encode()], [], e, bstats)
    assert sorted(cols) == ["match", "ok"] and cols["ok"] == v.CheckBlob(blob, e)
    assert bstats == stats and stats["host"] > 0 and stats["scanned"] > 0
    assert masks_of(cols, len(toks)) == [b or 0 for b, _ in rows]
    assert list(cols["ok"]) == [int(err is None) for _, err in rows]
    es = [e, expected(J, CC.T0 + 7200), J.Expected(Now=lambda: CC.T0 + 30, SigningAlgorithms=["RS256"], Issuer="other")]
    which = [i % 3 for i in range(len(toks))]
    estats = {}
    each = v.MatchBatchArgsEach(toks, reqs, es, which, [nonces], [], estats)
    alone = [v.MatchBatchArgs(toks, reqs, [nonces], [], x) for x in es]
    assert each == [alone[w][i] for i, w in enumerate(which)]
    assert [err for _, err in each] == v.CheckBatchEach(toks, es, which)
    assert estats["scanned"] > 0 and estats["host"] > 0 and 0 < sum(err is None for _, err in each) < len(toks) - 3
    ecols = v.MatchBlobArgsEach(blob, reqs, es, array.array("I", which), ["\n".join(nonces).encode()], [])
    assert masks_of(ecols, len(toks)) == [b or 0 for b, _ in each]
    assert list(ecols["ok"]) == [int(err is None) for _, err in each]
