"""CPU check of tests/ed_point_model.py, the bit-exact model of the Ed25519
point kernels: at every key-table tier, for the one-lane chain order and the
split's (two and four lanes), (X/Z, Y/Z) of the model's limbs equals
[S]B + [k](-A) computed by double-and-add on big integers
(tests/table_model.py), Z is not zero, and every limb of every intermediate
and final point is inside the "normalized" bound of fe25519.hpp (limb i <
2^w_i, limb 1 < 2^25 + 2^13).  Tokens: ed_point_model.tokens -- the recoding
edges, zero scalars, one-lane scalars, single digits, a sum that is the
neutral element, equal B-side and A-side sums -- on an ordinary key, and a few
on a key of order 8 and on A = B / A = -B.  This is what makes limb equality
with the device meaningful (tests/test_gpu_ed_point_exact.py)."""
import random

import pytest

from tests import ed_point_model as E
from tests import scalar_model as M
from tests import table_model as T

SECRET = 0x0b5e55ed25519c0ffee0ddba11ca11ab1e5eed0fa11edbee5f00d5ca1ab1e123 % E.L


def neg(A):
    return (-A[0] % E.P, A[1])


def order8_point():
    for y in range(2, 100):
        A = T.ed_decode_key(y.to_bytes(32, "little"))
        if A is None:
            continue
        Q = T.ed_mul(E.L, A)
        if T.ed_mul(4, Q) != T.ED_IDENTITY:
            return Q
    raise AssertionError("no point of order 8 found")


def run_tokens(w, negA, toks):
    """every token through both chain orders; returns the failures"""
    dg = {tag: E.digits(S, k, w) for tag, S, k in toks}
    need = set().union(*(E.named_entries(*d) for d in dg.values()))
    tab = {0: E.entry_words(T.ed_base(), M.ED_WB, [(x, ad) for s, x, ad in need if s == 0]),
           1: E.entry_words(negA, w, [(x, ad) for s, x, ad in need if s == 1])}
    entry = lambda side, win, ad: tab[side][(win, ad)]
    bad = []
    for tag, S, k in toks:
        sd, kd = dg[tag]
        assert M.digits_value(sd, M.ED_WB) == S and M.digits_value(kd, w) == k
        ref = E.reference(S, k, negA)
        for form, lanes in (("one-lane", 1), ("split-2", 2), ("split-4", 4)):
            trace = []
            out = E.chain_one_lane(sd, kd, entry, trace) if lanes == 1 else E.chain_split(sd, kd, entry, lanes, trace)
            if not E.same_point(out[:3], ref):
                bad.append((w, tag, form, "not [S]B + [k](-A)"))
            if (E.B.value(out[3]) * E.B.value(out[2]) - E.B.value(out[0]) * E.B.value(out[1])) % E.P:
                bad.append((w, tag, form, "T Z != X Y"))
            if not all(E.normalized(v) for Q in trace + [out] for v in Q):
                bad.append((w, tag, form, "a limb outside the normalized bound"))
    return bad


@pytest.mark.parametrize("w", M.ED_WA)
def test_model_equals_big_integers(w):
    A = T.ed_mul(SECRET, T.ed_base())
    toks = E.tokens(w, 4, SECRET, seed=1)
    bad = run_tokens(w, neg(A), toks)
    assert not bad, (len(bad), bad[:8])
    # the special cases are what they claim to be
    by = {tag: (S, k) for tag, S, k in toks}
    for tag in ("sum-neutral-0", "sum-neutral-small"):
        S, k = by[tag]
        X, Y, Z, _ = E.reference(S, k, neg(A))
        assert X % E.P == 0 and (Y - Z) % E.P == 0
    for tag in ("sides-equal-0", "sides-equal-small"):
        S, k = by[tag]
        assert T.ed_mul(S, T.ed_base()) == T.ed_mul(k, neg(A))


def test_model_on_special_keys():
    """a key of order 8 (every entry of the windows above 0 is the neutral
    element), A = B with S = k (the sum is neutral; at equal widths each window
    pair cancels), A = -B with S = k (the same point twice)"""
    rng = random.Random(8)
    Bp = T.ed_base()
    for w in (24, 16):
        toks = [("r%d" % i, rng.randrange(E.L), rng.randrange(E.L)) for i in range(3)] + [("k=8", 5, 8), ("z", 0, 0)]
        assert not run_tokens(w, neg(order8_point()), toks)
        same = [("S=k-%d" % i, u, u) for i, u in enumerate([rng.randrange(E.L), 1, 1 << 48, E.L - 1])]
        for A in (Bp, neg(Bp)):
            assert not run_tokens(w, neg(A), same)
    # A = B, S = k at W = 24: after every window pair the accumulator is the neutral element again
    u = rng.randrange(E.L)
    sd, kd = E.digits(u, u, 24)
    assert sd == kd
    need = [(x, ad) for s, x, ad in E.named_entries(sd, kd) if s == 0]
    tab = {0: E.entry_words(Bp, 24, need), 1: E.entry_words(neg(Bp), 24, need)}
    trace = []
    E.chain_one_lane(sd, kd, lambda s, x, ad: tab[s][(x, ad)], trace)
    assert len(trace) == 2 * sum(1 for d in sd if d)
    for Q in trace[1::2]:
        X, Y, Z, _ = (E.B.value(v) % E.P for v in Q)
        assert X == 0 and Y == Z != 0


def test_neutral_token_and_single_digits():
    """what falls out of the model for the tokens whose addition order is
    stepped through by hand: S = k = 0 leaves the one-lane chain at exactly
    (0, 1, 1); the split adds neutral elements with add_ext and ends on
    limbs that still say X = 0, Y = Z; one digit is one Niels addition of the
    entry to (0, 1, 1, 0), the entry's own point"""
    none = lambda *a: pytest.fail("a zero digit named an entry")
    sd, kd = E.digits(0, 0, 16)
    assert E.chain_one_lane(sd, kd, none) == E.neutral()
    for lanes in (2, 4):
        X, Y, Z, Tt = E.chain_split(sd, kd, none, lanes)
        # (E = B - A is 2p limb by limb there, so X and T come out as a multiple of p, not as zero limbs)
        assert E.B.value(X) % E.P == 0 and E.B.value(Tt) % E.P == 0 and X != [0] * 10
        assert Y == Z and E.B.value(Z) % E.P != 0
        assert all(E.normalized(v) for v in (X, Y, Z, Tt))
    Bp = T.ed_base()
    for d in (1, -1, 2, -(1 << 23) + 1, 1 << 23):
        ent = E.entry_words(Bp, 24, [(0, abs(d))])[(0, abs(d))]
        out = E.add_niels(E.neutral(), ent, d)
        want = T.ed_mul(abs(d), Bp)
        want = want if d > 0 else neg(want)
        assert E.same_point(out[:3], T._ed_ext(want)) and all(E.normalized(v) for v in out)


def test_add_niels_sign_selection_matters():
    """the model tells +entry from -entry, and entry ad from ad - 1 (what the device test relies on)"""
    Bp = T.ed_base()
    ents = E.entry_words(Bp, 24, [(0, 2), (0, 3)])
    plus, minus = E.add_niels(E.neutral(), ents[(0, 3)], 3), E.add_niels(E.neutral(), ents[(0, 3)], -3)
    assert plus != minus and plus != E.add_niels(E.neutral(), ents[(0, 2)], 3)
    assert E.add_niels(plus, ents[(0, 3)], 0) is plus
