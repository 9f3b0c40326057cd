"""Crafted RSA encodings and length sweeps for the RSA padding checks and the
device SHA stages (tests/test_rsa_em_reference.py, tests/test_gpu_rsa_em.py).

With the private parts of the committed test keys (tests/golden/craft_keys.json,
made by tests/golden/make_craft_keys.py) any encoded message EM < n can be
signed, so the verifier meets s^e mod n == EM for near-miss encodings: every
single-byte deviation of EMSA-PKCS1-v1_5, every PSS salt length, every PSS
reject rule.  The references are plain Python (hashlib, pow); signing is CRT
modexp, through the system libcrypto's BN_mod_exp where ctypes finds one (the
2048-bit lists alone cost ~20 s with pow) and pow otherwise, every signature
checked with pow(s, e, n) == EM.  The expected verdict of a case
is known by construction, `em_accepts` restates Go's rule independently, and
the C oracle is the third opinion.

  sign_raw(key, em)                        EM^d mod n by CRT
  pkcs1_em / pss_em                        the encodings (any salt, forced bits)
  em_accepts(alg, key_bits, em, msg)       rsa.VerifyPKCS1v15 / rsa.VerifyPSS with
                                           PSSSaltLengthAuto on the decrypted EM
                                           
  cases()                                  (name, alg, kid, msg, sig, expected), seeded
"""
import ctypes
import ctypes.util
import functools
import hashlib
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
HASH = {256: hashlib.sha256, 384: hashlib.sha384, 512: hashlib.sha512}
DIGESTINFO = {
    256: bytes.fromhex("3031300d060960864801650304020105000420"),
    384: bytes.fromhex("3041300d060960864801650304020205000430"),
    512: bytes.fromhex("3051300d060960864801650304020305000440"),
}
# DigestInfo without the NULL parameters (17 bytes): a valid DER form that Go's exact compare rejects
DIGESTINFO_NONULL = {
    256: bytes.fromhex("302f300b0609608648016503040201" "0420"),
    384: bytes.fromhex("303f300b0609608648016503040202" "0430"),
    512: bytes.fromhex("304f300b0609608648016503040203" "0440"),
}
RSA_KIDS = ["rsa2047-a", "rsa2048-a", "rsa2049-b", "rsa3072-a", "rsa4096-a"]
SMALL_IN_MAX = 8192                      # kernels/common.hpp: longer inputs leave the one-launch path


class RsaKey:
    def __init__(self, kid, d):
        self.kid = kid
        self.n, self.e, self.d = int(d["n"], 16), int(d["e"]), int(d["d"], 16)
        self.p, self.q = int(d["p"], 16), int(d["q"], 16)
        self.bits = self.n.bit_length()
        self.k = (self.bits + 7) // 8
        self.dp, self.dq, self.qinv = self.d % (self.p - 1), self.d % (self.q - 1), pow(self.q, -1, self.p)


@functools.lru_cache(maxsize=None)
def keys():
    d = json.load(open(os.path.join(HERE, "golden", "craft_keys.json")))
    out = {kid: RsaKey(kid, v) for kid, v in d["rsa"].items()}
    out["ed-a"] = bytes.fromhex(d["ed25519"]["ed-a"]["seed"])
    return out


@functools.lru_cache(maxsize=None)
def _bn():
    """libcrypto's BN_mod_exp through ctypes where the system has it (about 10x
    Python's pow at these sizes; the whole list signs in seconds); else None."""
    try:
        path = ctypes.util.find_library("crypto")
        L = ctypes.CDLL(path) if path else None
        if L is None:
            return None
        vp = ctypes.c_void_p
        L.BN_new.restype = L.BN_CTX_new.restype = L.BN_bin2bn.restype = vp
        L.BN_bin2bn.argtypes = [ctypes.c_char_p, ctypes.c_int, vp]
        L.BN_mod_exp.argtypes = [vp, vp, vp, vp, vp]
        L.BN_num_bits.argtypes = [vp]
        L.BN_bn2bin.argtypes = [vp, ctypes.c_char_p]
        L.BN_free.argtypes = [vp]
        L.BN_CTX_free.argtypes = [vp]
        return L
    except (OSError, AttributeError):
        return None


def _modexp(a, e, m):
    L = _bn()
    if L is None:
        return pow(a, e, m)
    raw = [v.to_bytes((v.bit_length() + 7) // 8 or 1, "big") for v in (a, e, m)]
    bn = [L.BN_bin2bn(b, len(b), None) for b in raw]
    r, ctx = L.BN_new(), L.BN_CTX_new()
    try:
        if not (all(bn) and r and ctx) or L.BN_mod_exp(r, bn[0], bn[1], bn[2], ctx) != 1:
            return pow(a, e, m)
        out = ctypes.create_string_buffer((L.BN_num_bits(r) + 7) // 8 or 1)
        n = L.BN_bn2bin(r, out)
        return int.from_bytes(out.raw[:n], "big")
    finally:
        for b in bn + [r]:
            if b:
                L.BN_free(b)
        if ctx:
            L.BN_CTX_free(ctx)


def sign_raw(key, em: bytes):
    """EM^d mod n as k bytes (CRT), or None when EM >= n (no such signature)."""
    m = int.from_bytes(em, "big")
    if m >= key.n:
        return None
    m1, m2 = _modexp(m % key.p, key.dp, key.p), _modexp(m % key.q, key.dq, key.q)
    s = m2 + key.q * ((key.qinv * (m1 - m2)) % key.p)
    assert pow(s, key.e, key.n) == m
    return s.to_bytes(key.k, "big")


# ------------------------------------------------------------------ encodings
def pkcs1_em(k, hbits, msg, di=None, ff=None):
    """00 01 FF.. 00 DigestInfo H; `di` replaces the DigestInfo prefix, `ff`
    the length of the FF run (the result is then not k bytes: the caller pads)."""
    t = (DIGESTINFO[hbits] if di is None else di) + HASH[hbits](msg).digest()
    n_ff = k - len(t) - 3 if ff is None else ff
    return b"\x00\x01" + b"\xff" * n_ff + b"\x00" + t


def mgf1(seed, ln, h):
    out, c = b"", 0
    while len(out) < ln:
        out += h(seed + c.to_bytes(4, "big")).digest()
        c += 1
    return out[:ln]


def pss_em(bits, hbits, msg, salt, sep=1, db_set=None, salt_flip=None, h_flip=None, trailer=0xbc, top_or=0,
           lead=0):
    """EMSA-PSS-ENCODE for a `bits`-bit modulus, as k bytes.  Deviations:
    sep = the separator byte; db_set = {DB offset: byte} written into DB before
    masking; salt_flip = salt bit to flip in DB after H was computed; h_flip =
    (byte, mask) XORed into H in the EM; trailer; top_or = bits ORed into the
    first EM byte after the top bits were cleared; lead = the leading byte
    when k > emLen."""
    h = HASH[hbits]
    embits = bits - 1
    emlen, k = (embits + 7) // 8, (bits + 7) // 8
    hh = h(b"\x00" * 8 + h(msg).digest() + salt).digest()
    db = bytearray(b"\x00" * (emlen - len(salt) - len(hh) - 2) + bytes([sep]) + salt)
    for off, v in (db_set or {}).items():
        db[off] = v
    if salt_flip is not None:
        db[len(db) - len(salt) + salt_flip // 8] ^= 1 << (salt_flip % 8)
    masked = bytearray(x ^ y for x, y in zip(db, mgf1(hh, len(db), h)))
    masked[0] &= 0xff >> (8 * emlen - embits)
    masked[0] |= top_or
    if h_flip is not None:
        hh = bytearray(hh)
        hh[h_flip[0]] ^= h_flip[1]
    em = bytes(masked) + bytes(hh) + bytes([trailer])
    assert len(em) == emlen and k - emlen in (0, 1)
    return bytes([lead]) * (k - emlen) + em


# ------------------------------------------------------------------ the Go rule, restated
def em_accepts(alg, key_bits, em, msg):
    """Verdict of rsa.VerifyPKCS1v15 (RS*) / rsa.VerifyPSS with PSSSaltLengthAuto
    (PS*) given em = I2OSP(s^e mod n, k) and the message."""
    hbits = int(alg[2:])
    h = HASH[hbits]
    hashed = h(msg).digest()
    hlen = len(hashed)
    k = (key_bits + 7) // 8
    if len(em) != k:
        return False
    if alg.startswith("RS"):
        prefix = DIGESTINFO[hbits]
        tlen = len(prefix) + hlen
        if k < tlen + 11:
            return False
        ok = em[0] == 0 and em[1] == 1
        ok = ok and all(b == 0xff for b in em[2:k - tlen - 1])
        ok = ok and em[k - tlen - 1] == 0
        ok = ok and em[k - tlen:k - hlen] == prefix
        return ok and em[k - hlen:] == hashed
    embits = key_bits - 1
    emlen = (embits + 7) // 8
    if any(em[:k - emlen]):                      # m must fit in emLen bytes
        return False
    em = em[k - emlen:]
    if emlen < hlen + 2 or em[-1] != 0xbc:
        return False
    mdb, hh = em[:emlen - hlen - 1], em[emlen - hlen - 1:emlen - 1]
    bitmask = 0xff >> (8 * emlen - embits)
    if em[0] & ~bitmask & 0xff:
        return False
    db = bytearray(x ^ y for x, y in zip(mdb, mgf1(hh, len(mdb), h)))
    db[0] &= bitmask
    ps = db.find(b"\x01")                        # PSSSaltLengthAuto: the first 0x01 ...
    if ps < 0 or any(db[:ps]):                   # ... after zeros only
        return False
    return h(b"\x00" * 8 + hashed + bytes(db[ps + 1:])).digest() == hh


# ------------------------------------------------------------------ Ed25519 (RFC 8032), signing only
ED_P = 2**255 - 19
ED_L = 2**252 + 27742317777372353535851937790883648493
ED_D = (-121665 * pow(121666, ED_P - 2, ED_P)) % ED_P
ED_I = pow(2, (ED_P - 1) // 4, ED_P)


def _ed_recover_x(y, sign):
    xx = (y * y - 1) * pow(ED_D * y * y + 1, ED_P - 2, ED_P) % ED_P
    x = pow(xx, (ED_P + 3) // 8, ED_P)
    if (x * x - xx) % ED_P != 0:
        x = x * ED_I % ED_P
    assert (x * x - xx) % ED_P == 0
    return ED_P - x if x & 1 != sign else x


ED_BY = 4 * pow(5, ED_P - 2, ED_P) % ED_P
ED_B = (_ed_recover_x(ED_BY, 0), ED_BY, 1, _ed_recover_x(ED_BY, 0) * ED_BY % ED_P)


def _ed_add(P, Q):
    (X1, Y1, Z1, T1), (X2, Y2, Z2, T2) = P, Q
    A = (Y1 - X1) * (Y2 - X2) % ED_P
    B = (Y1 + X1) * (Y2 + X2) % ED_P
    C = T1 * 2 * ED_D * T2 % ED_P
    D = Z1 * 2 * Z2 % ED_P
    E, F, G, H = B - A, D - C, D + C, B + A
    return (E * F % ED_P, G * H % ED_P, F * G % ED_P, E * H % ED_P)


def _ed_mul(s, P):
    Q = (0, 1, 1, 0)
    while s > 0:
        if s & 1:
            Q = _ed_add(Q, P)
        P = _ed_add(P, P)
        s >>= 1
    return Q


def _ed_encode(P):
    X, Y, Z, _ = P
    zi = pow(Z, ED_P - 2, ED_P)
    x, y = X * zi % ED_P, Y * zi % ED_P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def ed_public(seed: bytes):
    h = hashlib.sha512(seed).digest()
    a = (int.from_bytes(h[:32], "little") & ((1 << 254) - 8)) | (1 << 254)
    return a, h[32:], _ed_encode(_ed_mul(a, ED_B))


def ed_sign(seed: bytes, msg: bytes) -> bytes:
    a, prefix, A = ed_public(seed)
    r = int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % ED_L
    R = _ed_encode(_ed_mul(r, ED_B))
    kk = int.from_bytes(hashlib.sha512(R + A + msg).digest(), "little") % ED_L
    return R + ((r + kk * a) % ED_L).to_bytes(32, "little")


# ------------------------------------------------------------------ the case list
def _pkcs_flip_positions(key, hbits, rng, n_ff):
    k, hlen = key.k, hbits // 8
    tlen = 19 + hlen
    pos = set(range(0, 9)) | set(range(k - tlen - 6, k - tlen + 5)) | set(range(k - hlen - 2, k - hlen + 2)) | \
        set(range(k - 4, k))
    ff_lo, ff_hi = 2, k - tlen - 1                    # the FF run is em[ff_lo:ff_hi]
    pos |= set(rng.sample(range(ff_lo + 7, ff_hi - 6), n_ff))
    return sorted(pos)


def _msg(rng, n):
    return bytes(rng.choices(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_.", k=n))


@functools.lru_cache(maxsize=None)
def cases(seed=0xC4AF7):
    """The whole list, signed once per process: tuples (name, alg, kid, msg,
    sig, expected).  A mutated EM >= n has no signature and is skipped; that
    can only happen to a mutation of byte 0 (byte 1 on the 2049-bit key)."""
    rng = random.Random(seed)
    K = keys()
    out, skipped, may_skip = [], [], [0]

    def add(name, alg, kid, msg, em, expected, touches_top=False):
        key = K[kid]
        assert len(em) == key.k, name
        may_skip[0] += bool(touches_top)
        sig = sign_raw(key, em)
        if sig is None:
            assert touches_top, name
            skipped.append(name)
            return
        out.append((name, alg, kid, msg, sig, int(expected)))

    def top(key, i):                                  # does a mutation of EM byte i reach the top of n?
        return i == 0 or (key.bits == 2049 and i == 1)

    # ---- EMSA-PKCS1-v1_5
    for kid in RSA_KIDS:
        key = K[kid]
        for hbits in (256, 384, 512):
            alg, tag = f"RS{hbits}", f"{kid}/RS{hbits}"
            msg = _msg(rng, 150 + rng.randrange(100))
            em = pkcs1_em(key.k, hbits, msg)
            add(f"{tag}/valid", alg, kid, msg, em, 1)
            if kid == "rsa2048-a" and hbits == 256:
                flips = [(i, x) for i in range(key.k) for x in (0x01, 0x80)]
            else:
                # thinned for the big keys (signing cost): fewer seeded FF-run positions
                n_ff = 16 if key.bits < 3000 else (6 if key.bits < 4000 or hbits == 256 else 2)
                flips = [(i, 0x01) for i in _pkcs_flip_positions(key, hbits, rng, n_ff)]
            for i, x in flips:
                bad = bytearray(em)
                bad[i] ^= x
                add(f"{tag}/flip{i}^{x:02x}", alg, kid, msg, bytes(bad), 0, top(key, i))
            # 00 00 01 FF.. 00 T: the run one byte short, everything shifted
            add(f"{tag}/shifted", alg, kid, msg, b"\x00" + pkcs1_em(key.k - 1, hbits, msg), 0)
            # 00 01 FFx8 00 T garbage: T not right-aligned
            short = pkcs1_em(0, hbits, msg, ff=8)
            add(f"{tag}/t-not-right-aligned", alg, kid, msg, short + bytes(rng.randrange(256) for _ in range(key.k - len(short))), 0)
            # DigestInfo without the NULL parameters (two more FF bytes)
            add(f"{tag}/digestinfo-no-null", alg, kid, msg,
                pkcs1_em(key.k, hbits, msg, di=DIGESTINFO_NONULL[hbits], ff=key.k - 17 - hbits // 8 - 3), 0)
            # T of another hash under this alg
            other = {256: 384, 384: 512, 512: 256}[hbits]
            add(f"{tag}/t-of-sha{other}", alg, kid, msg, pkcs1_em(key.k, other, msg), 0)

    # ---- EMSA-PSS: salt lengths
    for kid in RSA_KIDS:
        key = K[kid]
        emlen = (key.bits - 1 + 7) // 8
        for hbits in (256, 384, 512):
            alg, hlen = f"PS{hbits}", hbits // 8
            smax = emlen - hlen - 2
            if kid == "rsa2048-a":
                slens = list(range(0, smax + 1))
            else:
                slens = sorted(set(range(0, 6)) | {hlen - 1, hlen, hlen + 1} | set(range(smax - 5, smax + 1)))
                if key.bits > 4000 and hbits != 256:      # thinned (signing cost)
                    slens = [0, 1, 2, 3, hlen, smax - 3, smax - 2, smax - 1, smax]
            for sl in slens:
                msg = _msg(rng, 40 + rng.randrange(200))
                salt = bytes(rng.randrange(256) for _ in range(sl))
                add(f"{kid}/{alg}/salt{sl}", alg, kid, msg, pss_em(key.bits, hbits, msg, salt), 1)

    # ---- EMSA-PSS: every reject rule
    for kid in RSA_KIDS:
        key = K[kid]
        embits = key.bits - 1
        emlen = (embits + 7) // 8
        for hbits in ((256, 384, 512) if key.bits < 3000 else (256,)):
            alg, hlen, tag = f"PS{hbits}", hbits // 8, f"{kid}/PS{hbits}"
            msg = _msg(rng, 40 + rng.randrange(200))
            salt = bytes(rng.randrange(256) for _ in range(hlen))
            ps = emlen - 2 * hlen - 2
            B = functools.partial(pss_em, key.bits, hbits, msg, salt)
            add(f"{tag}/trailer-bd", alg, kid, msg, B(trailer=0xbd), 0)
            for bit in range(8):
                if (0xff >> (8 * emlen - embits)) & (1 << bit):
                    continue
                add(f"{tag}/topbit{bit}", alg, kid, msg, B(top_or=1 << bit), 0, key.k == emlen)
            if key.k > emlen:
                # 01 || EM is below n for about half of all salts: take the first salt that can be signed
                for _ in range(64):
                    em = pss_em(key.bits, hbits, msg, bytes(rng.randrange(256) for _ in range(hlen)), lead=1)
                    if int.from_bytes(em, "big") < key.n:
                        break
                add(f"{tag}/lead-nonzero", alg, kid, msg, em, 0, True)
            for off in (0, 1, 3, 4, ps - 1):
                add(f"{tag}/db{off}-nonzero", alg, kid, msg, B(db_set={off: 0x02}), 0)
            add(f"{tag}/sep-02", alg, kid, msg, B(sep=2), 0)
            add(f"{tag}/sep-00-empty-salt", alg, kid, msg, pss_em(key.bits, hbits, msg, b"", sep=0), 0)
            for name, i in (("first", 0), ("mid", hlen // 2), ("last", hlen - 1)):
                add(f"{tag}/h-{name}-bit", alg, kid, msg, B(h_flip=(i, 1 << rng.randrange(8))), 0)
            add(f"{tag}/flipped-salt-bit", alg, kid, msg, B(salt_flip=rng.randrange(8 * hlen)), 0)
            add(f"{tag}/other-message", alg, kid, msg, pss_em(key.bits, hbits, msg + b"x", salt), 0)

    # ---- signing-input length sweep, correctly signed
    key = K["rsa2048-a"]
    for hbits, lens in ((256, list(range(1, 301)) + [SMALL_IN_MAX - 1, SMALL_IN_MAX, SMALL_IN_MAX + 1]),
                        (384, range(100, 261)), (512, range(100, 261))):
        for ln in lens:
            msg = _msg(rng, ln)
            add(f"len/RS{hbits}/{ln}", f"RS{hbits}", "rsa2048-a", msg, pkcs1_em(key.k, hbits, msg), 1)
    seed_ed = K["ed-a"]
    for ln in list(range(1, 9)) + list(range(40, 73)) + list(range(104, 137)) + list(range(168, 201)):
        msg = _msg(rng, ln)
        out.append((f"len/EdDSA/{ln}", "EdDSA", "ed-a", msg, ed_sign(seed_ed, msg), 1))

    assert len(skipped) <= may_skip[0]
    return tuple(out), tuple(skipped)


def summary(cs):
    """case counts per class, for the record"""
    cnt = {}
    for name, alg, kid, _, _, exp in cs:
        cls = "len-sweep" if name.startswith("len/") else ("pkcs1" if alg.startswith("RS") else "pss")
        key = (cls, kid, "accept" if exp else "reject")
        cnt[key] = cnt.get(key, 0) + 1
    return cnt
