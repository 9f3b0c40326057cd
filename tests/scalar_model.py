"""Plain big-integer model of the scalar-level stages between prep and the point
sums (no GPU, no project code): what k_ec_scalar_batch (ecdsa_impl.hpp), the
Ed25519 k = H mod L / S check / recode (ed25519.hip) and k_ed_finish compute,
restated from the rules they implement.

ECDSA, go-jose ecEncrypterVerifier.verifyPayload -> crypto/ecdsa.Verify (SURVEY.md
R18-R22): the size of r and s comes from the alg (ES256 32, ES384 48, ES512 66
bytes), the curve from the key, with no check that they belong together;
r, s in [1, n-1]; e = the leftmost min(hash, curve) bytes of the digest as a
big-endian integer (the curves' bit lengths are multiples of 8, or longer than
any hash: no bit shift ever applies), reduced mod n; u1 = e / s, u2 = r / s.
The comb kernels then want u as signed W-bit digits, u = sum d_w 2^(W w).

Ed25519, crypto/ed25519.Verify (R23-R26): sig[63] & 0xE0 == 0 and S < L;
k = SHA-512(R || A || M) as a little-endian integer mod L; accept iff the
encoding of R' = (X/Z, Y/Z) equals sig[:32] byte for byte."""

CLS_P256, CLS_P384, CLS_P521 = 4, 5, 6
ES256, ES384, ES512 = 7, 8, 9

EC_N = {
    CLS_P256: 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551,
    CLS_P384: int("ffffffffffffffffffffffffffffffffffffffffffffffffc7634d81f4372ddf"
                  "581a0db248b0a77aecec196accc52973", 16),
    CLS_P521: int("01ff" + "ff" * 31 + "fa51868783bf2f966b7fcc0148f709a5d03bb5c9b8899c47aebb6fb71e91386409", 16),
}
EC_BITS = {CLS_P256: 256, CLS_P384: 384, CLS_P521: 521}
EC_BYTES = {CLS_P256: 32, CLS_P384: 48, CLS_P521: 66}
EC_CLS = {"P-256": CLS_P256, "P-384": CLS_P384, "P-521": CLS_P521}
ES_SIZE = {ES256: 32, ES384: 48, ES512: 66}          # bytes of r (and of s), by alg
ES_HASH = {ES256: 32, ES384: 48, ES512: 64}          # digest bytes, by alg
# comb widths (ecdsa.hpp): the generator's, and the key-table tiers widest first
EC_WG = {CLS_P256: 26, CLS_P384: 24, CLS_P521: 20}
EC_WQ = {CLS_P256: (26, 24, 22, 20), CLS_P384: (24, 20, 18, 16), CLS_P521: (20, 18, 16)}

ED_P = 2**255 - 19
ED_L = 2**252 + 27742317777372353535851937790883648493
ED_WB = 24                                           # base-point comb width (ed25519.hpp)
ED_WA = (24, 22, 20, 18, 16)                         # key-table tiers


def ec_windows(cls, w):
    """windows per scalar at width w: ceil((bits + 2) / w) (ecdsa.hpp ec_windows_w)"""
    return (EC_BITS[cls] + 2 + w - 1) // w


def ec_digit_rows(cls):
    return ec_windows(cls, EC_WG[cls]) + ec_windows(cls, EC_WQ[cls][-1])


def ed_windows(w):
    return (253 + 1 + w - 1) // w


def recode(u, w, nwin, carry_at_half):
    """Signed w-bit digits of u, lowest window first.  carry_at_half: a window
    value (with the carry in) of exactly 2^(w-1) carries (ECDSA: digits in
    [-2^(w-1), 2^(w-1))); otherwise only a larger one does (Ed25519: digits in
    (-2^(w-1), 2^(w-1)]).  Returns (digits, carry out of the last window)."""
    half, c, out = 1 << (w - 1), 0, []
    for i in range(nwin):
        v = ((u >> (w * i)) & ((1 << w) - 1)) + c
        c = int(v >= half if carry_at_half else v > half)
        out.append(v - (c << w))
    return out, c


def digits_value(digits, w):
    return sum(d << (w * i) for i, d in enumerate(digits))


def ec_e(cls, alg, digest):
    """e of crypto/ecdsa hashToInt, reduced mod n; digest: the alg's whole hash"""
    assert len(digest) == ES_HASH[alg]
    return int.from_bytes(digest[:min(ES_HASH[alg], EC_BYTES[cls])], "big") % EC_N[cls]


def ec_range_ok(cls, r, s):
    n = EC_N[cls]
    return 1 <= r < n and 1 <= s < n


def ec_scalars(cls, alg, r, s, digest):
    """(u1, u2) of an ECDSA signature on a key of curve `cls`, or None where
    crypto/ecdsa.Verify returns false before any point arithmetic.  r, s: the
    alg's ES_SIZE-byte big-endian integers."""
    if not ec_range_ok(cls, r, s):
        return None
    n = EC_N[cls]
    w = pow(s, -1, n)
    return ec_e(cls, alg, digest) * w % n, r * w % n


def ed_k(digest):
    """k = SHA-512(R || A || M) mod L, the digest read little-endian"""
    assert len(digest) == 64
    return int.from_bytes(digest, "little") % ED_L


def ed_s_ok(sbytes):
    """sig[32:64]: sig[63] & 0xE0 == 0 and S < L"""
    assert len(sbytes) == 32
    return (sbytes[31] & 0xE0) == 0 and int.from_bytes(sbytes, "little") < ED_L


def ed_patterns(w):
    """scalars below L whose windows at width w hit the recoding's edges"""
    k = 252 // w                              # the highest window holding bits of a scalar < ED_L
    sh, half, full = w * k, 1 << (w - 1), (1 << w) - 1
    ntop = ED_L >> sh

    def build(low, top):
        u = sum(v << (w * i) for i, v in enumerate(low)) | (min(top, ntop - 1) << sh)
        assert 0 < u < ED_L
        return u

    return [build([half - 1] * k, half - 1), build([half] * k, half), build([half + 1] * k, half + 1),
            build([full] * k, ntop - 1),                                      # 2^252 - 1: a carry into a full top window
            build([full] * (k - 1) + [half], ntop - 1),
            build([(half + 1 if i % 2 else 0) for i in range(k)], 1),         # zero windows
            (half + 1) << (w * (k // 2)), half << (w * (k // 2)),             # a lone digit
            1, half, half + 1, ED_L - 1]


def ed_encode(X, Y, Z):
    """canonical 32-byte encoding of the projective point (X : Y : Z), Z != 0 mod p"""
    zi = pow(Z % ED_P, -1, ED_P)
    x, y = X * zi % ED_P, Y * zi % ED_P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")
