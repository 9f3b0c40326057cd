"""ClaimSet.Add under Validator.MatchBatchArgs / MatchBlobArgs: signed RS256
tokens held against a deny-list with InSet("sid", s) and AnyElementIn("groups",
g), before and after s.Add(...) and g.Add(...).

The tokens, the requirements and the reference are
tests/test_gpu_match_set_batch.py's: ok / err are ValidateBatch's, and every bit
is the plain-Python evaluation on the claims map ValidateBatch returns, against
the members the set holds at that moment.  Among the tokens are a tampered one
(no bits), payloads with an escape (the host path), and the last Add turns the
set host-only.
"""
import pytest

from tests.test_gpu_match_set_batch import (GROUPS, J, REVOKED, check_rows, crafted, expected, masks_of,  # noqa: F401 (fixtures)
                                            requires)

pytestmark = pytest.mark.gpu


def rows_and_blob(v, crafted, reqs, e, revoked, groups, stats=None):
    """MatchBatchArgs' rows, checked against the Python evaluation, and MatchBlobArgs' columns against the rows"""
    _, toks, kinds, nonces = crafted
    rows = v.MatchBatchArgs(toks, reqs, [nonces], [], e, stats)
    bits = check_rows(v, crafted, rows, e, revoked=revoked, groups=groups)
    cols = v.MatchBlobArgs("\n".join(toks).encode(), reqs, ["\n".join(nonces).encode()], [], e)
    assert masks_of(cols, len(toks)) == [b or 0 for b in bits]
    assert list(cols["ok"]) == [int(err is None) for _, err in rows]
    return bits


def test_add_acts_on_the_next_call_on_both_paths(crafted, J):
    v, toks, kinds, nonces = crafted
    first = REVOKED[:20]                                                          # jti-0 .. jti-38
    revoked, groups = v.NewClaimSet(first, seed=11), v.NewClaimSet(GROUPS[:1])
    reqs, e = requires(J, revoked, groups), expected(J)
    verified = sum(k != "tampered" for k in kinds)
    host = sum(k in ("escape", "escape-group") for k in kinds)
    stats = {}
    before = rows_and_blob(v, crafted, reqs, e, first, GROUPS[:1], stats)
    assert stats == {"scanned": verified - host, "host": host}
    i0 = revoked.info()
    # the rest of the list, with repeats and residents among them
    assert revoked.Add(REVOKED + first[:5]) == len(set(REVOKED)) - 20
    assert groups.Add(GROUPS) == 2
    i1 = revoked.info()
    assert (i1["n"], i1["seed"], i1["host_only"]) == (len(set(REVOKED)), 11, False) and i1["generation"] > i0["generation"]
    assert i1["nslots"] >= 2 * i1["n"] and len(revoked) == len(set(REVOKED)) and groups.info()["n"] == 3
    stats = {}
    after = rows_and_blob(v, crafted, reqs, e, REVOKED, GROUPS, stats)
    assert stats == {"scanned": verified - host, "host": host}                   # still decided on the device
    flipped = [i for i, (a, b) in enumerate(zip(before, after)) if a is not None and (a ^ b) & 1]
    assert len(flipped) >= 3 and any(kinds[i] == "escape" for i in flipped)      # the host path sees the added members too
    assert any(a is not None and (a ^ b) & 2 for a, b in zip(before, after))     # "ops" came with the add to groups
    assert all((a is None) == (b is None) for a, b in zip(before, after)) and before[kinds.index("tampered")] is None
    # the same rows as the whole list loaded at once
    whole = v.NewClaimSet(REVOKED, seed=11)
    assert [b for b, _ in v.MatchBatchArgs(toks, requires(J, whole, groups), [nonces], [], e)] == after
    whole.Close()
    # nothing new: no new generation
    assert revoked.Add(REVOKED[:7]) == 0 and revoked.Add([]) == 0 and revoked.info()["generation"] == i1["generation"]
    # a member the device does not take: host-only from here on, and the payload that holds it is found
    assert revoked.Add(["jti-é", "jti-1"]) == 2 and revoked.info()["host_only"] and revoked.info()["nslots"] == 0
    stats = {}
    ho = rows_and_blob(v, crafted, reqs, e, REVOKED + ["jti-é", "jti-1"], GROUPS, stats)
    assert stats == {"scanned": 0, "host": verified} and ho != after
    assert revoked.Add(["late"]) == 1 and len(revoked) == len(set(REVOKED)) + 3
    with pytest.raises(ValueError):
        revoked.Add(["nul\0"])
    revoked.Close()
    with pytest.raises(ValueError):
        revoked.Add(["x"])
    groups.Close()
