"""Bit-exact model of the Ed25519 point kernels (kernels/ed25519.hip k_ed_point,
k_ed_point_pf, k_ed_point_split): R' = [S]B + [k](-A) as a chain of Niels
additions of comb-table entries in the radix-2^25.5 field of fe25519.hpp.

Field elements are lists of ten limbs; fe::mul is tools/fe25519_bounds.py
model_mul, and add / sub / add_dbl / sub_dbl / neg are restated limb-wise
(32-bit wrap-around included, so that the model stays defined on any input).
A point is [X, Y, Z, T].  tests/test_ed_point_model.py holds the model to
big-integer arithmetic; tests/test_gpu_ed_point_exact.py holds the device
code to the model limb for limb.

`tokens(w, ...)` is the token set both tests run: random (S, k), the recoding
edges, zero scalars, scalars living on one lane of the split, and the special
cases of the addition law."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fe25519_bounds as B  # noqa: E402

from tests import scalar_model as M  # noqa: E402
from tests import table_model as T  # noqa: E402

P, L = M.ED_P, M.ED_L
U32 = 1 << 32
FE_L = B.L
# 2d mod p, canonical radix-2^25.5 limbs (ed25519.hip add_ext)
D2 = [0x2b2f159, 0x1a6e509, 0x22add7a, 0x0d4141d, 0x0038052, 0x0f3d130, 0x3407977, 0x19ce331, 0x1c56dff, 0x0901b67]
# "normalized" (fe25519.hpp): limb i < 2^w_i, limb 1 < 2^25 + 2^13
NORM_BOUND = [(1 << w) + ((1 << 13) if i == 1 else 0) for i, w in enumerate(B.WID)]


# ------------------------------------------------------------------ fe25519.hpp, limb-wise
def fe_add(a, b):
    return [(x + y) % U32 for x, y in zip(a, b)]


def fe_sub(a, b):
    return [(x + q - y) % U32 for x, y, q in zip(a, b, B.P2)]


def fe_add_dbl(a, b):
    return [(2 * x + y) % U32 for x, y in zip(a, b)]


def fe_sub_dbl(a, b):
    return [(2 * x + q - y) % U32 for x, y, q in zip(a, b, B.P2)]


def fe_neg(b):
    return [(q - y) % U32 for y, q in zip(b, B.P2)]


def neutral():
    """(0, 1, 1, 0) as fe::set_small leaves it"""
    one = [1] + [0] * (FE_L - 1)
    return [[0] * FE_L, list(one), list(one), [0] * FE_L]


def normalized(limbs):
    return all(0 <= x < b for x, b in zip(limbs, NORM_BOUND))


# ------------------------------------------------------------------ the additions
def add_niels(Pt, ent, d):
    """add_entry + add_niels: Pt + sign(d) * entry.  ent: the entry's words
    (y+x, y-x, 2dxy: ten limbs each); d: the signed digit (0: no addition)."""
    if d == 0:
        return Pt
    ypx, ymx, t2d = list(ent[0:10]), list(ent[10:20]), list(ent[20:30])
    if d < 0:                                     # -(x, y) = (-x, y): swap y+x / y-x, negate 2dxy
        ypx, ymx, t2d = ymx, ypx, fe_neg(t2d)
    X, Y, Z, Tt = Pt
    C = B.model_mul(t2d, Tt)
    F, G = fe_sub_dbl(Z, C), fe_add_dbl(Z, C)
    A = B.model_mul(ymx, fe_sub(Y, X))
    Bb = B.model_mul(ypx, fe_add(Y, X))
    E, H = fe_sub(Bb, A), fe_add(Bb, A)
    return [B.model_mul(F, E), B.model_mul(H, G), B.model_mul(F, G), B.model_mul(H, E)]


def add_ext(Pt, Qt):
    """ed25519.hip add_ext(R, P, Q): extended + extended, operand for operand"""
    X1, Y1, Z1, T1 = Pt
    X2, Y2, Z2, T2 = Qt
    t = B.model_mul(T2, D2)
    C = B.model_mul(t, T1)
    t = B.model_mul(Z1, Z2)
    Dd = fe_add(t, t)
    F, G = fe_sub(Dd, C), fe_add(Dd, C)
    A = B.model_mul(fe_sub(Y2, X2), fe_sub(Y1, X1))
    Bb = B.model_mul(fe_add(Y2, X2), fe_add(Y1, X1))
    E, H = fe_sub(Bb, A), fe_add(Bb, A)
    return [B.model_mul(F, E), B.model_mul(H, G), B.model_mul(F, G), B.model_mul(H, E)]


# ------------------------------------------------------------------ the chains
def _digit(ds, w):
    return ds[w] if w < len(ds) else 0


def chain_one_lane(S_digits, k_digits, entry, trace=None):
    """k_ed_point / k_ed_point_pf: for w = 0 .. NW - 1 the B window w, then the
    -A window w, from the neutral element.  entry(side, w, ad): the words of
    entry ad = |d| of window w of the base table (side 0) or the key's (side
    1); it is asked only for digits that are not zero.  trace: a list that
    receives every intermediate point."""
    Pt = neutral()
    for w in range(max(len(S_digits), len(k_digits))):
        for side, ds in ((0, S_digits), (1, k_digits)):
            d = _digit(ds, w)
            if d:
                Pt = add_niels(Pt, entry(side, w, abs(d)), d)
                if trace is not None:
                    trace.append(Pt)
    return Pt


def chain_split(S_digits, k_digits, entry, lanes, trace=None):
    """k_ed_point_split<WA, lanes>: lane `par` of side 0 (S, base table) and of
    side 1 (k, key table) sums the windows par, par + H, ... (H = lanes / 2);
    with four lanes the two partials of each side meet first (lanes xor 1: the
    even lane's add_ext(P, P, Q)), then lane 0 adds side 0 + side 1."""
    assert lanes in (2, 4)
    H = lanes // 2
    nw = max(len(S_digits), len(k_digits))
    part = []
    for side, ds in ((0, S_digits), (1, k_digits)):
        for par in range(H):
            Pt = neutral()
            for w in range(par, nw, H):
                d = _digit(ds, w)
                if d:
                    Pt = add_niels(Pt, entry(side, w, abs(d)), d)
            part.append(Pt)
    if trace is not None:
        trace.extend(part)
    if lanes == 4:
        part = [add_ext(part[0], part[1]), add_ext(part[2], part[3])]
        if trace is not None:
            trace.extend(part)
    return add_ext(part[0], part[1])


# ------------------------------------------------------------------ digits, entries, reference
def digits(S, k, w):
    """(S digits at the base width, k digits at the key-table width w)"""
    sd, c1 = M.recode(S, M.ED_WB, M.ed_windows(M.ED_WB), False)
    kd, c2 = M.recode(k, w, M.ed_windows(w), False)
    assert c1 == 0 and c2 == 0
    return sd, kd


def named_entries(sd, kd):
    """the (side, window, |digit|) triples a token's digits name"""
    return {(side, w, abs(d)) for side, ds in ((0, sd), (1, kd)) for w, d in enumerate(ds) if d}


def entry_words(point, W, pairs):
    """{(w, ad): the 32 words of entry ad of window w} of the width-W comb table of the affine point"""
    if not pairs:
        return {}
    aff = T.want_many(T.CLS_ED25519, point, W, pairs)
    return {wd: T.ed_encode(T.ed_niels(Q)) for wd, Q in aff.items()}


def reference(S, k, negA):
    """[S]B + [k](-A) by double-and-add on big integers: extended (X, Y, Z, T)"""
    return T._ed_add(T._ed_mul(S, T._ed_ext(T.ed_base())), T._ed_mul(k, T._ed_ext(negA)))


def same_point(limbs_xyz, ref):
    """(X/Z, Y/Z) of the limbs equals the reference point, and Z is not zero"""
    X, Y, Z = (B.value(v) % P for v in limbs_xyz)
    return Z != 0 and ref[2] % P != 0 and (X * ref[2] - ref[0] * Z) % P == 0 and (Y * ref[2] - ref[1] * Z) % P == 0


# ------------------------------------------------------------------ the token set
def _lane_scalar(rng, w, par, H):
    """a scalar below L whose non-zero digits at width w all sit in windows = par mod H"""
    nw, half = M.ed_windows(w), 1 << (w - 1)
    ws = [i for i in range(par, nw, H) if w * i < 250]
    u = 0
    for n, i in enumerate(ws):
        room = min(half, (1 << (250 - w * i)) - 1)       # the value stays below 2^250 < L
        v = half if (n == 1 and room == half) else rng.randrange(1, room + 1)
        u |= v << (w * i)
    d, c = M.recode(u, w, nw, False)
    assert c == 0 and 0 < u < L and all((x != 0) <= (i % H == par) for i, x in enumerate(d))
    return u


def tokens(w, nrand, secret, seed, lanes=4):
    """[(tag, S, k)] for a key A = secret * B at key-table width w: every named
    edge token, then nrand random pairs.  All S, k are below L."""
    rng = random.Random(seed * 1000 + w)
    rnd = lambda: rng.randrange(1, L)
    H = lanes // 2
    out = [("S=k=0", 0, 0), ("k=0", rnd(), 0), ("S=0", 0, rnd())]
    pk, ps = M.ed_patterns(w), M.ed_patterns(M.ED_WB)
    for i, u in enumerate(pk):
        out.append(("k-pattern-%d" % i, rnd(), u))
    for i, u in enumerate(ps):
        out.append(("S-pattern-%d" % i, u, pk[(i + 5) % len(pk)]))
    # scalars on one lane of the split: the other lanes hand add_ext the neutral element
    ev_s, od_s = _lane_scalar(rng, M.ED_WB, 0, H), _lane_scalar(rng, M.ED_WB, H - 1, H)
    ev_k, od_k = _lane_scalar(rng, w, 0, H), _lane_scalar(rng, w, H - 1, H)
    out += [("lane-S0-k1", ev_s, od_k), ("lane-S1-k0", od_s, ev_k), ("lane-S0-only", ev_s, 0), ("lane-k1-only", 0, od_k)]
    # a single non-zero digit
    out += [("one-digit-S", 1 << M.ED_WB, 0), ("one-digit-k", 0, 3 << w), ("one-digit-each", 5, 7),
            ("one-digit-top-S", 1 << 250, 0), ("one-digit-top-k", 0, 1 << 251)]
    # the addition law's special cases: [S]B + [k](-A) = (S - k a) B
    for i in range(2):
        k = rnd()
        out.append(("sum-neutral-%d" % i, k * secret % L, k))           # [S]B = [k]A
        out.append(("sides-equal-%d" % i, -k * secret % L, k))          # [S]B = [k](-A): the last addition doubles
    out += [("sum-neutral-small", secret, 1), ("sides-equal-small", L - secret, 1)]
    out += [("random-%d" % i, rnd(), rnd()) for i in range(nrand)]
    assert all(0 <= S < L and 0 <= k < L for _, S, k in out)
    return out
