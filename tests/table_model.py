"""Plain big-integer model of the comb tables (no GPU, no project code): what
k_ec_table_base_* / k_ec_table_* (ecdsa_impl.hpp) and k_ed_table_base_* /
k_ed_table_* (ed25519.hip) leave in HBM, restated from the definition.

A table of comb width W for a point P holds NWIN windows of NE = 2^(W-1)
entries; entry e = w * NE + (d - 1) is d * 2^(W w) * P in affine coordinates:

  P-256          x then y, 8 little-endian 32-bit words each, canonical
                 Montgomery form with R = 2^280 (store_entry, ec_packed);
                 stride 16 words
  P-384, P-521   x then y, L = 15 / 20 limbs of 28 bits each, canonical
                 Montgomery form with R = 2^(28 L); stride (2L + 3) & ~3
  Ed25519        the Niels form (y + x, y - x, 2 d x y): three canonical
                 values of 10 radix-2^25.5 limbs (niels_entry / mont_to_fe:
                 limb i at bit ceil(25.5 i), 26 / 25 bits wide); stride 32

Words of the stride past these are padding and are not looked at.  The
decoders assert canonicity (every limb within its width, every value below
p).  For an Ed25519 key P is -A, A decoded from the 32 key bytes by the rule
of Go's edwards25519 Point.SetBytes (DESIGN R24): the sign bit is taken off,
y is reduced mod p (non-canonical encodings are accepted), x^2 =
(y^2 - 1) / (d y^2 + 1) must be a square, and the root whose low bit equals
the sign bit is taken -- x = 0 with the sign bit set is accepted as x = 0."""
import random

from tests import scalar_model as M

CLS_P256, CLS_P384, CLS_P521, CLS_ED25519 = M.CLS_P256, M.CLS_P384, M.CLS_P521, 7
SLICE = 1 << 23                                  # entries per launch of a sliced build (kernels/tables.hpp)
LIMB_BITS = 28

EC = {
    CLS_P256: dict(
        p=2**256 - 2**224 + 2**192 + 2**96 - 1, L=10,
        b=0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b,
        gx=0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296,
        gy=0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5),
    CLS_P384: dict(
        p=2**384 - 2**128 - 2**96 + 2**32 - 1, L=15,
        b=int("b3312fa7e23ee7e4988e056be3f82d19181d9c6efe8141120314088f5013875a"
              "c656398d8a2ed19d2a85c8edd3ec2aef", 16),
        gx=int("aa87ca22be8b05378eb1c71ef320ad746e1d3b628ba79b9859f741e082542a38"
               "5502f25dbf55296c3a545e3872760ab7", 16),
        gy=int("3617de4a96262c6f5d9e98bf9292dc29f8f41dbd289a147ce9da3113b5f0b8c0"
               "0a60b1ce1d7e819d7a431d7c90ea0e5f", 16)),
    CLS_P521: dict(
        p=2**521 - 1, L=20,
        b=int("0051953eb9618e1c9a1f929a21a0b68540eea2da725b99b315f3b8b489918ef1"
              "09e156193951ec7e937b1652c0bd3bb1bf073573df883d2c34f1ef451fd46b503f00", 16),
        gx=int("00c6858e06b70404e9cd9e3ecb662395b4429c648139053fb521f828af606b4d"
               "3dbaa14b5e77efe75928fe1dc127a2ffa8de3348b3c1856a429bf97e7e31c2e5bd66", 16),
        gy=int("011839296a789a3bc0045c8a5fb42c7d1bd998f54449579b446817afbd17273e"
               "662c97ee72995ef42640c550b9013fad0761353c7086a272c24088be94769fd16650", 16)),
}
ED_P, ED_L = M.ED_P, M.ED_L
ED_D = -121665 * pow(121666, -1, ED_P) % ED_P
ED_SQRT_M1 = pow(2, (ED_P - 1) // 4, ED_P)
ED_STRIDE = 32
FE_SHIFT = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]     # limb i of radix 2^25.5 sits at bit ceil(25.5 i)
FE_BITS = [26, 25, 26, 25, 26, 25, 26, 25, 26, 25]
ED_IDENTITY = (0, 1)


def is_ec(cls):
    return cls in EC


def stride(cls):
    if cls == CLS_ED25519:
        return ED_STRIDE
    return 16 if cls == CLS_P256 else (2 * EC[cls]["L"] + 3) & ~3


def windows(cls, w):
    return M.ed_windows(w) if cls == CLS_ED25519 else M.ec_windows(cls, w)


def ec_generator(cls):
    return EC[cls]["gx"], EC[cls]["gy"]


def ec_on_curve(cls, P):
    p, b = EC[cls]["p"], EC[cls]["b"]
    x, y = P
    return 0 <= x < p and 0 <= y < p and (y * y - (x * x * x - 3 * x + b)) % p == 0


# ------------------------------------------------------------------ raw entry layouts
def _mont_r(cls):
    return 1 << (LIMB_BITS * EC[cls]["L"])


def ec_encode(cls, P):
    """affine (x, y) -> the stride's words (padding zero)"""
    p, L = EC[cls]["p"], EC[cls]["L"]
    vals = [v * _mont_r(cls) % p for v in P]
    if cls == CLS_P256:
        return [(v >> (32 * q)) & 0xFFFFFFFF for v in vals for q in range(8)]
    out = [(v >> (LIMB_BITS * j)) & ((1 << LIMB_BITS) - 1) for v in vals for j in range(L)]
    return out + [0] * (stride(cls) - len(out))


def ec_decode(cls, words):
    """the stride's words -> affine (x, y); asserts canonical Montgomery form"""
    p, L = EC[cls]["p"], EC[cls]["L"]
    assert len(words) == stride(cls)
    if cls == CLS_P256:
        assert all(0 <= w < 2**32 for w in words)
        vals = [sum(words[8 * i + q] << (32 * q) for q in range(8)) for i in range(2)]
    else:
        assert all(0 <= w < (1 << LIMB_BITS) for w in words[:2 * L]), "a limb over 28 bits"
        vals = [sum(words[L * i + j] << (LIMB_BITS * j) for j in range(L)) for i in range(2)]
    assert all(v < p for v in vals), "a coordinate not below p"
    ri = pow(_mont_r(cls), -1, p)
    return tuple(v * ri % p for v in vals)


def fe_limbs(v):
    assert 0 <= v < 2**255
    return [(v >> s) & ((1 << b) - 1) for s, b in zip(FE_SHIFT, FE_BITS)]


def fe_value(limbs):
    assert len(limbs) == 10
    assert all(0 <= l < (1 << b) for l, b in zip(limbs, FE_BITS)), "a limb over its 26 / 25 bits"
    v = sum(l << s for l, s in zip(limbs, FE_SHIFT))
    assert v < ED_P, "a value not below p"
    return v


def ed_niels(P):
    """affine (x, y) -> (y + x, y - x, 2 d x y)"""
    x, y = P
    return (y + x) % ED_P, (y - x) % ED_P, 2 * ED_D * x * y % ED_P


def ed_encode(N):
    """Niels triple -> the stride's words (padding zero)"""
    return [l for v in N for l in fe_limbs(v)] + [0, 0]


def ed_decode(words):
    """the stride's words -> Niels triple; asserts canonical limbs and values"""
    assert len(words) == ED_STRIDE
    return tuple(fe_value(words[10 * i:10 * i + 10]) for i in range(3))


def encode(cls, P):
    return ed_encode(ed_niels(P)) if cls == CLS_ED25519 else ec_encode(cls, P)


def decode(cls, words):
    """what an entry's words hold, in the form `expected` gives"""
    return ed_decode(words) if cls == CLS_ED25519 else ec_decode(cls, words)


def expected(cls, P):
    """the affine point P in the form `decode` returns"""
    return ed_niels(P) if cls == CLS_ED25519 else P


# ------------------------------------------------------------------ short Weierstrass, a = -3, Jacobian
def _jdbl(p, P):
    if P is None:
        return None
    X, Y, Z = P
    if Y == 0:
        return None
    yy = Y * Y % p
    s = 4 * X * yy % p
    zz = Z * Z % p
    m = 3 * (X - zz) * (X + zz) % p
    X3 = (m * m - 2 * s) % p
    return X3, (m * (s - X3) - 8 * yy * yy) % p, 2 * Y * Z % p


def _jadd(p, P, Q):
    if P is None:
        return Q
    if Q is None:
        return P
    X1, Y1, Z1 = P
    X2, Y2, Z2 = Q
    z1z1, z2z2 = Z1 * Z1 % p, Z2 * Z2 % p
    u1, u2 = X1 * z2z2 % p, X2 * z1z1 % p
    s1, s2 = Y1 * Z2 * z2z2 % p, Y2 * Z1 * z1z1 % p
    if u1 == u2:
        return _jdbl(p, P) if s1 == s2 else None
    h, r = (u2 - u1) % p, (s2 - s1) % p
    hh = h * h % p
    hhh, v = h * hh % p, u1 * hh % p
    X3 = (r * r - hhh - 2 * v) % p
    return X3, (r * (v - X3) - s1 * hhh) % p, h * Z1 * Z2 % p


def _jmul(p, k, P):
    acc = None
    for bit in range(k.bit_length() - 1, -1, -1):
        acc = _jdbl(p, acc)
        if (k >> bit) & 1:
            acc = _jadd(p, acc, P)
    return acc


def _batch_inverse(p, zs):
    """1 / z for every z (none zero) with one inversion"""
    pre, acc = [], 1
    for z in zs:
        pre.append(acc)
        acc = acc * z % p
    inv = pow(acc, -1, p)
    out = [0] * len(zs)
    for i in range(len(zs) - 1, -1, -1):
        out[i] = inv * pre[i] % p
        inv = inv * zs[i] % p
    return out


def ec_mul(cls, k, P):
    """k * P for affine P = (x, y); None is the point at infinity"""
    p = EC[cls]["p"]
    R = _jmul(p, k, (P[0], P[1], 1))
    if R is None:
        return None
    zi = pow(R[2], -1, p)
    return R[0] * zi * zi % p, R[1] * zi * zi * zi % p


# ------------------------------------------------------------------ edwards25519, extended coordinates
def _ed_add(P, Q):
    """the unified a = -1 addition: complete on the whole curve (d is a non-square)"""
    (X1, Y1, Z1, T1), (X2, Y2, Z2, T2) = P, Q
    A = (Y1 - X1) * (Y2 - X2) % ED_P
    B = (Y1 + X1) * (Y2 + X2) % ED_P
    C = T1 * 2 * ED_D * T2 % ED_P
    D = Z1 * 2 * Z2 % ED_P
    E, F, G, H = B - A, D - C, D + C, B + A
    return E * F % ED_P, G * H % ED_P, F * G % ED_P, E * H % ED_P


def _ed_mul(k, P):
    acc = (0, 1, 1, 0)
    for bit in range(k.bit_length() - 1, -1, -1):
        acc = _ed_add(acc, acc)
        if (k >> bit) & 1:
            acc = _ed_add(acc, P)
    return acc


def _ed_ext(P):
    return P[0], P[1], 1, P[0] * P[1] % ED_P


def ed_mul(k, P):
    """k * P for affine P = (x, y); the identity is (0, 1)"""
    X, Y, Z, _ = _ed_mul(k, _ed_ext(P))
    zi = pow(Z, -1, ED_P)
    return X * zi % ED_P, Y * zi % ED_P


def ed_on_curve(P):
    x, y = P
    return (-x * x + y * y - 1 - ED_D * x * x * y * y) % ED_P == 0


def ed_base():
    y = 4 * pow(5, -1, ED_P) % ED_P
    return ed_decode_key(y.to_bytes(32, "little"))


def ed_decode_key(key):
    """A = (x, y) of 32 key bytes by Go's Point.SetBytes rule (see the module
    docstring), or None where the key is invalid (x^2 a non-square)"""
    assert len(key) == 32
    v = int.from_bytes(key, "little")
    sign, y = v >> 255, (v & (2**255 - 1)) % ED_P
    xx = (y * y - 1) * pow(ED_D * y * y + 1, -1, ED_P) % ED_P
    x = pow(xx, (ED_P + 3) // 8, ED_P)
    if x * x % ED_P != xx:
        x = x * ED_SQRT_M1 % ED_P
    if x * x % ED_P != xx:
        return None
    if x & 1 != sign:
        x = -x % ED_P
    return x, y


def ed_key_point(key):
    """the point an Ed25519 key's comb table is built from: -A, or None for an invalid key"""
    A = ed_decode_key(key)
    return None if A is None else (-A[0] % ED_P, A[1])


# ------------------------------------------------------------------ table entries
def want(cls, P, W, w, d):
    """d * 2^(W w) * P, affine (EC: never infinity for P of prime order and d 2^(W w) below n)"""
    return want_many(cls, P, W, [(w, d)])[(w, d)]


def want_many(cls, P, W, pairs):
    """{(w, d): d * 2^(W w) * P affine} for every pair: the window bases by a
    chain of doublings, d times a base in W bits, one inversion for all"""
    pairs = sorted(set(pairs))
    top = max(w for w, _ in pairs)
    if cls == CLS_ED25519:
        dbl, mul, base, p = (lambda Q: _ed_add(Q, Q)), _ed_mul, _ed_ext(P), ED_P
    else:
        p = EC[cls]["p"]
        dbl, mul, base = (lambda Q: _jdbl(p, Q)), (lambda k, Q: _jmul(p, k, Q)), (P[0], P[1], 1)
    bases = [base]
    for _ in range(top):
        Q = bases[-1]
        for _ in range(W):
            Q = dbl(Q)
        bases.append(Q)
    proj = [mul(d, bases[w]) for w, d in pairs]
    assert None not in proj, "an entry at infinity"
    zi = _batch_inverse(p, [Q[2] for Q in proj])
    if cls == CLS_ED25519:
        aff = [(Q[0] * z % p, Q[1] * z % p) for Q, z in zip(proj, zi)]
    else:
        aff = [(Q[0] * z * z % p, Q[1] * z * z * z % p) for Q, z in zip(proj, zi)]
    return dict(zip(pairs, aff))


def sample_entries(W, nwin, seed=0x7AB1E):
    """The entries a table check reads, as sorted entry indices e = w NE + (d - 1):
    d in {1, 2, 3, NE - 1, NE} of every window, the table's first and last
    entry, the entries around every multiple of the build slice (k 2^23 - 1,
    k 2^23, k 2^23 + 1 for 0 < k 2^23 < NWIN NE), and 64 seeded random (w, d)."""
    ne = 1 << (W - 1)
    total = nwin * ne
    es = {0, total - 1}
    for w in range(nwin):
        es |= {w * ne + d - 1 for d in (1, 2, 3, ne - 1, ne)}
    for k in range(1, (total - 1) // SLICE + 1):
        es |= {e for e in (k * SLICE - 1, k * SLICE, k * SLICE + 1) if e < total}
    rng = random.Random(seed)
    for _ in range(64):
        es.add(rng.randrange(nwin) * ne + rng.randrange(1, ne + 1) - 1)
    return sorted(es)


def runs(es):
    """sorted indices -> [(first, count)] of consecutive runs"""
    out = []
    for e in es:
        if out and out[-1][0] + out[-1][1] == e:
            out[-1][1] += 1
        else:
            out.append([e, 1])
    return [tuple(r) for r in out]


def table_mismatches(cls, P, W, nwin, read, es=None):
    """Compare the entries `es` (default sample_entries) of a table of width W
    built from the affine point P with the reference.  read(first, count)
    returns count * stride raw words.  Returns [(w, d, what)] of every entry
    that is not canonical or not exactly d * 2^(W w) * P."""
    ne, st = 1 << (W - 1), stride(cls)
    es = sample_entries(W, nwin) if es is None else es
    ref = want_many(cls, P, W, [(e // ne, e % ne + 1) for e in es])
    bad = []
    for first, count in runs(es):
        words = read(first, count)
        assert len(words) == count * st
        for i in range(count):
            w, d = (first + i) // ne, (first + i) % ne + 1
            try:
                got = decode(cls, words[i * st:(i + 1) * st])
            except AssertionError as e:
                bad.append((w, d, "not canonical: " + str(e)))
                continue
            if got != expected(cls, ref[(w, d)]):
                bad.append((w, d, "wrong value"))
    return bad
