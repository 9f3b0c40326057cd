"""The comb-table reference of tests/table_model.py against facts that do not
depend on it (CPU only): the entry layouts round-trip and reject non-canonical
words, the curve arithmetic knows the group orders, Ed25519 key decoding
follows Go's SetBytes rule, and a table entry is the plain scalar multiple."""
import random

import pytest

from tests import craft
from tests import scalar_model as M
from tests import table_model as T

EC_CLS = [T.CLS_P256, T.CLS_P384, T.CLS_P521]
ALL_CLS = EC_CLS + [T.CLS_ED25519]


def _neg(cls, P):
    return (P[0], -P[1] % T.EC[cls]["p"])


@pytest.mark.parametrize("cls", EC_CLS)
def test_ec_layout_round_trip(cls):
    rng = random.Random(cls)
    p = T.EC[cls]["p"]
    vals = [0, 1, p - 1, 2, p - 2] + [rng.randrange(p) for _ in range(50)]
    for x in vals:
        for y in (vals[0], vals[1], vals[2], rng.randrange(p)):
            words = T.ec_encode(cls, (x, y))
            assert len(words) == T.stride(cls) and all(0 <= w < 2**32 for w in words)
            assert T.ec_decode(cls, words) == (x, y)
    assert [T.stride(c) for c in EC_CLS] == [16, 32, 40]
    # 1 in Montgomery form is R mod p: x then y, lowest word / limb first
    r = (1 << (28 * T.EC[cls]["L"])) % p
    words = T.ec_encode(cls, (1, 0))
    if cls == T.CLS_P256:
        assert words[:8] == [(r >> (32 * q)) & 0xFFFFFFFF for q in range(8)] and words[8:] == [0] * 8
    else:
        L = T.EC[cls]["L"]
        assert words[:L] == [(r >> (28 * j)) & 0xFFFFFFF for j in range(L)] and words[L:] == [0] * (T.stride(cls) - L)


@pytest.mark.parametrize("cls", EC_CLS)
def test_ec_decoder_asserts_canonicity(cls):
    p, L = T.EC[cls]["p"], T.EC[cls]["L"]
    words = T.ec_encode(cls, (5, 7))
    if cls == T.CLS_P256:
        over = [(p >> (32 * q)) & 0xFFFFFFFF for q in range(8)]               # x = p itself
        with pytest.raises(AssertionError):
            T.ec_decode(cls, over + words[8:])
        with pytest.raises(AssertionError):
            T.ec_decode(cls, words[:8] + over)
    else:
        over = [(p >> (28 * j)) & 0xFFFFFFF for j in range(L)]
        with pytest.raises(AssertionError):
            T.ec_decode(cls, over + words[L:])
        with pytest.raises(AssertionError):
            T.ec_decode(cls, words[:L] + over + words[2 * L:])
        lazy = list(words)
        lazy[0] += 1 << 28                                                      # same value, a limb too wide
        lazy[1] -= 1
        with pytest.raises(AssertionError):
            T.ec_decode(cls, lazy)
        padded = list(words)
        for j in range(2 * L, T.stride(cls)):
            padded[j] = 0xA5A5A5A5                                              # padding is not looked at
        assert T.ec_decode(cls, padded) == (5, 7)


def test_ed_layout_round_trip():
    rng = random.Random(25519)
    p = T.ED_P
    vals = [0, 1, p - 1, 2, 2**255 - 20, 2**26 - 1, 2**26] + [rng.randrange(p) for _ in range(100)]
    for a in vals:
        N = (a, vals[rng.randrange(len(vals))], rng.randrange(p))
        words = T.ed_encode(N)
        assert len(words) == 32 == T.stride(T.CLS_ED25519)
        assert T.ed_decode(words) == N
    assert T.FE_SHIFT == [(51 * i + 1) // 2 for i in range(10)]               # ceil(25.5 i)
    assert [b - a for a, b in zip(T.FE_SHIFT, T.FE_SHIFT[1:] + [255])] == T.FE_BITS
    assert T.fe_limbs(p - 1) == [2**26 - 20] + [2**25 - 1, 2**26 - 1] * 4 + [2**25 - 1]
    # the identity's Niels form
    assert T.ed_niels(T.ED_IDENTITY) == (1, 1, 0)
    assert T.ed_encode((1, 1, 0)) == [1] + [0] * 9 + [1] + [0] * 9 + [0] * 12


def test_ed_decoder_asserts_canonicity():
    words = T.ed_encode((3, 4, 5))
    with pytest.raises(AssertionError):                                         # the value p: limbs in range
        T.ed_decode([2**26 - 19] + [2**25 - 1, 2**26 - 1] * 4 + [2**25 - 1] + words[10:])
    lazy = list(words)
    lazy[10] += 1 << 26
    lazy[11] -= 1
    with pytest.raises(AssertionError):
        T.ed_decode(lazy)
    wide = list(words)
    wide[21] = 1 << 25                                                          # an odd limb holds 25 bits
    with pytest.raises(AssertionError):
        T.ed_decode(wide)
    padded = list(words)
    padded[30] = padded[31] = 0xA5A5A5A5
    assert T.ed_decode(padded) == (3, 4, 5)


@pytest.mark.parametrize("cls", EC_CLS)
def test_ec_group_order(cls):
    G, n = T.ec_generator(cls), M.EC_N[cls]
    assert T.ec_on_curve(cls, G)
    assert T.ec_mul(cls, n - 1, G) == _neg(cls, G)
    assert T.ec_mul(cls, n, G) is None
    assert T.ec_mul(cls, n + 1, G) == G
    two = T.ec_mul(cls, 2, G)
    assert T.ec_on_curve(cls, two) and T.ec_mul(cls, 3, G) == T.ec_mul(cls, (n + 3) % n + n, G)
    # a + b the long way round: addition of distinct points and of a point to itself
    p = T.EC[cls]["p"]
    J = lambda P: (P[0], P[1], 1)
    s = T._jadd(p, J(two), J(G))
    zi = pow(s[2], -1, p)
    assert (s[0] * zi * zi % p, s[1] * zi**3 % p) == T.ec_mul(cls, 3, G)
    assert T._jadd(p, J(G), J(G)) == T._jdbl(p, J(G)) and T._jadd(p, J(G), J(_neg(cls, G))) is None


def test_ed_group_order_and_base_point():
    B = T.ed_base()
    assert B == (craft.ED_B[0], craft.ED_B[1]) and B[0] & 1 == 0 and T.ed_on_curve(B)
    assert T.ED_D == craft.ED_D
    assert T.ed_mul(T.ED_L, B) == T.ED_IDENTITY
    assert T.ed_mul(T.ED_L - 1, B) == (-B[0] % T.ED_P, B[1])
    assert T.ed_mul(0, B) == T.ED_IDENTITY and T.ed_mul(1, B) == B


def test_ed_public_key_decodes_to_seed_scalar_times_b():
    for seed in (bytes(32), bytes(range(32)), craft.keys()["ed-a"]):
        a, _, pub = craft.ed_public(seed)
        A = T.ed_decode_key(pub)
        assert A == T.ed_mul(a, T.ed_base())
        assert T.ed_key_point(pub) == (-A[0] % T.ED_P, A[1])


def test_ed_key_decoding_follows_setbytes():
    p = T.ED_P
    enc = lambda y, sign=0: (y | (sign << 255)).to_bytes(32, "little")
    assert T.ed_decode_key(enc(1)) == (0, 1)
    assert T.ed_decode_key(enc(1, 1)) == (0, 1)                  # x = 0 with the sign bit: accepted
    assert T.ed_decode_key(enc(p + 1)) == (0, 1)                 # non-canonical y, reduced
    assert T.ed_decode_key(enc(p - 1)) == (0, p - 1)             # order 2
    x4 = T.ed_decode_key(enc(0))                                 # order 4: x^2 = -1
    assert x4[1] == 0 and x4[0] * x4[0] % p == p - 1 and x4[0] & 1 == 0
    assert T.ed_decode_key(enc(0, 1)) == (p - x4[0], 0)
    assert T.ed_mul(2, (0, p - 1)) == T.ED_IDENTITY and T.ed_mul(2, x4) == (0, p - 1)
    # a y whose x^2 is a non-square: invalid, whatever the sign bit
    bad = [y for y in range(2, 40) if T.ed_decode_key(enc(y)) is None]
    assert bad and all(T.ed_decode_key(enc(y, 1)) is None for y in bad)
    for y in bad:
        xx = (y * y - 1) * pow(T.ED_D * y * y + 1, -1, p) % p
        assert pow(xx, (p - 1) // 2, p) == p - 1                 # Euler: not a square
    good = [y for y in range(2, 40) if y not in bad]
    for y in good:
        for s in (0, 1):
            A = T.ed_decode_key(enc(y, s))
            assert T.ed_on_curve(A) and A[0] & 1 == s and A[1] == y


@pytest.mark.parametrize("cls", ALL_CLS)
def test_want_is_the_plain_scalar_multiple(cls):
    rng = random.Random(100 + cls)
    if cls == T.CLS_ED25519:
        P, mul, widths = T.ed_key_point(craft.ed_public(bytes(range(32)))[2]), T.ed_mul, M.ED_WA
    else:
        k = rng.randrange(1, M.EC_N[cls])
        P, mul, widths = T.ec_mul(cls, k, T.ec_generator(cls)), (lambda s, Q: T.ec_mul(cls, s, Q)), M.EC_WQ[cls]
    for W in widths:
        assert T.want(cls, P, W, 0, 1) == P
        nwin, ne = T.windows(cls, W), 1 << (W - 1)
        pairs = [(0, 2), (0, ne), (1, 1), (nwin - 1, 1), (nwin - 1, ne), (nwin // 2, ne - 1),
                 (rng.randrange(nwin), rng.randrange(1, ne + 1))]
        got = T.want_many(cls, P, W, pairs)
        for w, d in pairs:
            assert got[(w, d)] == mul(d << (W * w), P), (W, w, d)


def test_want_on_small_order_points():
    p = T.ED_P
    assert T.want(T.CLS_ED25519, T.ED_IDENTITY, 16, 3, 1 << 15) == T.ED_IDENTITY
    assert T.want(T.CLS_ED25519, (0, p - 1), 16, 0, 3) == (0, p - 1)          # order 2: odd multiples
    assert T.want(T.CLS_ED25519, (0, p - 1), 16, 1, 3) == T.ED_IDENTITY
    x4 = T.ed_decode_key(bytes(32))
    assert T.want(T.CLS_ED25519, x4, 16, 0, 3) == (p - x4[0], 0)


def test_sample_set():
    for cls, W in [(T.CLS_P256, 26), (T.CLS_P256, 20), (T.CLS_P384, 24), (T.CLS_P521, 16), (T.CLS_ED25519, 24),
                   (T.CLS_ED25519, 16)]:
        nwin, ne = T.windows(cls, W), 1 << (W - 1)
        total = nwin * ne
        es = T.sample_entries(W, nwin)
        assert es == sorted(set(es)) and es[0] == 0 and es[-1] == total - 1
        for w in range(nwin):
            assert {w * ne, w * ne + 1, w * ne + 2, w * ne + ne - 2, w * ne + ne - 1} <= set(es)
        k = 1
        while k * T.SLICE < total:
            assert {k * T.SLICE - 1, k * T.SLICE} <= set(es) and (k * T.SLICE + 1 in es or k * T.SLICE + 1 == total)
            k += 1
        assert (k - 1 > 0) == (total > T.SLICE)
        assert len(es) <= 5 * nwin + 2 + 3 * (k - 1) + 64
        assert sum(c for _, c in T.runs(es)) == len(es) and all(a + c <= total for a, c in T.runs(es))
    assert T.runs([0, 1, 2, 7, 9, 10]) == [(0, 3), (7, 1), (9, 2)]


def test_table_mismatches_sees_a_wrong_entry():
    """the comparison itself: a model table passes; one wrong, one swapped and one non-canonical entry are reported"""
    cls, W = T.CLS_P384, 16
    P = T.ec_mul(cls, 12345, T.ec_generator(cls))
    nwin, ne, st = T.windows(cls, W), 1 << 15, T.stride(cls)
    es = [0, 1, 2, ne - 1, ne, 5 * ne + 7]
    ref = T.want_many(cls, P, W, [(e // ne, e % ne + 1) for e in es])
    table = {e: T.ec_encode(cls, ref[(e // ne, e % ne + 1)]) for e in es}
    read = lambda first, count: [w for e in range(first, first + count) for w in table[e]]
    assert T.table_mismatches(cls, P, W, nwin, read, es) == []
    table[1] = T.ec_encode(cls, ref[(0, 3)])
    x, y = ref[(1, 1)]
    table[ne] = T.ec_encode(cls, (y, x))
    table[5 * ne + 7] = [0xA5A5A5A5] * st
    bad = T.table_mismatches(cls, P, W, nwin, read, es)
    assert [(w, d) for w, d, _ in bad] == [(0, 2), (1, 1), (5, 8)]
    assert bad[2][2].startswith("not canonical")
