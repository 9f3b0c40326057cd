"""Exact parity of the batched ECDSA scalar stage (ecdsa_impl.hpp
k_ec_scalar_batch: Montgomery's trick over B tokens per thread, one inversion
per block through mp::block_inv) with a big-integer model
(tests/scalar_model.py), digit for digit, through the test hook tk_ec_scalar
(cap_amd/csrc/tests/tk_ec_scalar.hip).  Production picks B > 1 only from
262,144 padded tokens upward, so the chain tests run the kernel at B = 1 and
tell accept from reject only; here, at B = 1, 2, 3 and 16, one and four waves
per block, every key-table width, a class range that does not start at 0:

  * for every live token the device accepts: the generator rows reconstruct
    u1 = e / s and the key rows u2 = r / s exactly, every digit in
    [-2^(W-1), 2^(W-1)), key rows past the width's windows still poison,
    status still ST_OK;
  * for every live token the model rejects: ST_REJECT (digits not asserted);
  * padding lanes: status untouched; slots outside [begin, end): untouched;
  * the exception counter: 0 after exc_reset = 1, unchanged after 0.

Rejected tokens (s or r of 0, n, n + 1, all ones; status already ST_REJECT; an
invalid key; padding) sit at the first, a middle and the last position of a
thread's chain in every wave of a block, between valid neighbours whose digits
must stay exact.  (With the s = 1 substitution of a rejected token removed, one
s = 0 zeroes the product of its whole block: every four-wave case here fails,
at B = 1 too; a prefix product read from the wrong column fails from B = 2.)
Every assertion is exact equality."""
import ctypes
import os
import random

import numpy as np
import pytest

from tests import scalar_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_OK, ST_REJECT = 0, 1
JOB_PAD, WAVE, DIG_ROWS, EC_S_ROW = 15, 64, 16, 32
SIG_ROWS = EC_S_ROW + 17
POISON = 0xA5A5A5A5
ST_POISON = 0xA5                      # status_in of padding lanes and of slots outside the launch
NAMES = {M.CLS_P256: "p256", M.CLS_P384: "p384", M.CLS_P521: "p521"}


@pytest.fixture(scope="module")
def tk():
    L = ctypes.CDLL(os.path.join(ROOT, "cap_amd", "libcapjwt_tk.so"))
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.tk_ec_scalar.argtypes = [ctypes.c_int] * 4 + [i64] * 3 + [vp, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int,
                                                             ctypes.c_uint32, vp, vp, vp]
    L.tk_ec_scalar.restype = ctypes.c_int
    return L


class Tok:
    """one live token: alg, r, s (integers of the rows prep would leave), the
    alg's whole digest, the status byte it arrives with, the key's validity"""

    def __init__(self, alg, r, s, digest, tag, status=ST_OK, key_ok=True):
        self.alg, self.r, self.s, self.digest, self.tag, self.status, self.key_ok = alg, r, s, digest, tag, status, key_ok

    def scalars(self, cls):
        if self.status != ST_OK or not self.key_ok:
            return None
        return M.ec_scalars(cls, self.alg, self.r, self.s, self.digest)


def native_alg(cls):
    return {M.CLS_P256: M.ES256, M.CLS_P384: M.ES384, M.CLS_P521: M.ES512}[cls]


def rand_digest(rng, alg):
    return bytes(rng.randrange(256) for _ in range(M.ES_HASH[alg]))


def rand_valid(rng, cls, alg=None, tag="rand"):
    alg = alg or native_alg(cls)
    n = M.EC_N[cls]
    top = min(n, 1 << (8 * M.ES_SIZE[alg]))
    return Tok(alg, rng.randrange(1, top), rng.randrange(1, top), rand_digest(rng, alg), tag)


def digest_of_e(rng, cls, alg, e):
    """a digest whose leftmost min(hash, curve) bytes are e"""
    hb = min(M.ES_HASH[alg], M.EC_BYTES[cls])
    return e.to_bytes(hb, "big") + bytes(rng.randrange(256) for _ in range(M.ES_HASH[alg] - hb))


def chosen(rng, cls, u1, u2, tag):
    """a token of the curve's own alg with e / s = u1 and r / s = u2 (u2 != 0)"""
    alg, n = native_alg(cls), M.EC_N[cls]
    ebits = 8 * min(M.ES_HASH[alg], M.EC_BYTES[cls])
    if u1 == 0:
        e, s = 0, rng.randrange(1, n)
    else:
        e = rng.randrange(1, 1 << ebits)
        while e % n == 0:
            e = rng.randrange(1, 1 << ebits)
        s = e * pow(u1, -1, n) % n
    r = u2 * s % n
    t = Tok(alg, r, s, digest_of_e(rng, cls, alg, e), tag)
    assert t.scalars(cls) == (u1 % n, u2 % n)
    return t


def patterns(cls, w):
    """scalars in (0, n) whose windows at width w hit the recoding's edges"""
    n = M.EC_N[cls]
    k = (M.EC_BITS[cls] - 1) // w            # the highest window that holds bits of a scalar < n
    assert k + 1 <= M.ec_windows(cls, w)
    sh = w * k
    half, ntop = 1 << (w - 1), n >> sh       # ntop: that window of n (all ones for these curves)
    assert ntop >= 1

    def build(low, top):
        assert len(low) == k
        u = sum(v << (w * i) for i, v in enumerate(low)) | (min(top, ntop - 1) << sh)
        assert 0 < u < n
        return u

    out = {
        "max-digit": build([half - 1] * k, half - 1),                    # every window 2^(W-1) - 1: no carry
        "carry-chain": build([half] * k, half),                          # every window 2^(W-1): a carry through all
        "ones": build([(1 << w) - 1] * k, ntop - 1),
        "zero-windows": build([(half + 5 if i % 2 else 0) for i in range(k)], 1),
        "lone-digit": (half - 3) << (w * (k // 2)),
        "one": 1,
        "half": half,                                                    # digits -2^(W-1), +1
        "n-1": n - 1,
    }
    # a full top window with a carry in: the top window as n has it, the
    # window below at 2^(W-1)
    full = (ntop << sh) | (half << (sh - w))
    out["top-carry"] = full if full < n else build([0] * (k - 1) + [half], ntop - 1)
    for u in out.values():
        assert 0 < u < n
    return out


def pool(cls, wq, seed):
    """the special tokens of a (curve, key width), then 200 random ones"""
    rng = random.Random(seed)
    n, cb, nat = M.EC_N[cls], M.EC_BYTES[cls], native_alg(cls)
    toks = []

    def valid(alg=None):
        return rand_valid(rng, cls, alg)

    # range rejects of s and of r, and the accepted ends of the range
    ones = (1 << (8 * cb)) - 1
    for name, v in (("0", 0), ("n", n), ("n+1", n + 1), ("ones", ones)):
        t = valid(); t.s, t.tag = v, "rej-s=" + name; toks.append(t)
        t = valid(); t.r, t.tag = v, "rej-r=" + name; toks.append(t)
    for name, v in (("1", 1), ("n-1", n - 1)):
        t = valid(); t.s, t.tag = v, "ok-s=" + name; toks.append(t)
        t = valid(); t.r, t.tag = v, "ok-r=" + name; toks.append(t)
    t = valid(); t.status, t.tag = ST_REJECT, "rej-status"; toks.append(t)
    # e values: 0, n - 1, n, n + 1, an all-ones digest
    ebytes = min(M.ES_HASH[nat], cb)
    for name, e in (("0", 0), ("n-1", n - 1), ("n", n), ("n+1", n + 1), ("ones", (1 << (8 * ebytes)) - 1)):
        if e >> (8 * ebytes):
            continue                                  # P-521: n does not fit a 512-bit digest
        t = valid(); t.digest, t.tag = digest_of_e(rng, cls, nat, e), "e=" + name; toks.append(t)
    if cls == M.CLS_P521:
        # bits 521..527 of the top word, and bits past byte 66: both out of range
        for name, bit in (("bit521", 521), ("bit527", 527), ("bit528", 528), ("bit543", 543)):
            t = valid(); t.r |= 1 << bit; t.tag = "rej-r-" + name; toks.append(t)
            t = valid(); t.s |= 1 << bit; t.tag = "rej-s-" + name; toks.append(t)
        # ES256 / ES384 on the P-521 key: 32- / 48-byte r, s and digest
        for alg in (M.ES256, M.ES384):
            for _ in range(4):
                t = valid(alg); t.tag = "foreign-alg%d" % alg; toks.append(t)
            t = valid(alg); t.digest, t.tag = b"\xff" * M.ES_HASH[alg], "foreign-alg%d-e-ones" % alg; toks.append(t)
    else:
        # the other algs on this key: ES512's extra r / s words zero (accepted
        # when in range) or nonzero (rejected); e = the leftmost curve bytes
        for alg in (M.ES256, M.ES384, M.ES512):
            if alg == nat:
                continue
            for _ in range(4):
                t = valid(alg); t.tag = "foreign-alg%d" % alg; toks.append(t)
            t = valid(alg); t.digest, t.tag = b"\xff" * M.ES_HASH[alg], "foreign-alg%d-e-ones" % alg; toks.append(t)
            if M.ES_SIZE[alg] > cb:
                for name, bit in (("lo", 8 * cb), ("mid", 8 * cb + 37), ("hi", 8 * M.ES_SIZE[alg] - 1)):
                    t = valid(alg); t.r |= 1 << bit; t.tag = "rej-foreign-r-" + name; toks.append(t)
                    t = valid(alg); t.s |= 1 << bit; t.tag = "rej-foreign-s-" + name; toks.append(t)
    # chosen u1 (generator width) and u2 (key width) digit patterns
    p1, p2 = patterns(cls, M.EC_WG[cls]), patterns(cls, wq)
    for name in p1:
        toks.append(chosen(rng, cls, p1[name], p2[name], "u=" + name))
    toks.append(chosen(rng, cls, 0, p2["carry-chain"], "u1=0"))
    toks.append(chosen(rng, cls, p1["carry-chain"], p2["max-digit"], "u=carry/max"))
    for _ in range(200):
        toks.append(valid())
    return toks


def chain_spots(n, B, wpb, avoid):
    """(thread, j) pairs: the first, a middle and the last position of a chain
    in every wave of the first and of the last block that has work, each on a
    thread of its own whose chain holds no slot of `avoid` (where one exists)"""
    S = (n + B - 1) // B
    tpb = WAVE * wpb
    spots, used = [], set()
    for blk in sorted({0, (S - 1) // tpb}):
        for w in range(wpb):
            lo, hi = blk * tpb + w * WAVE, min(blk * tpb + (w + 1) * WAVE, S)
            for jn, jsel in enumerate(("first", "mid", "last")):
                free = [i for i in list(range(lo + 1 + 7 * jn, hi)) + list(range(lo, hi)) if i not in used]
                clean = [i for i in free if not avoid & set(range(i, n, S))]
                if not free:
                    continue
                i = (clean or free)[0]
                used.add(i)
                nb = len(range(i, n, S))                     # this thread's chain length (<= B)
                spots.append((i, {"first": 0, "mid": nb // 2, "last": nb - 1}[jsel]))
    return S, spots


def build_case(cls, wq, n, B, wpb, begin, npad, seed):
    """slots[npad]: None (padding lane) or a Tok; slots outside [begin, begin + n) are live and valid"""
    rng = random.Random(seed * 1000003 + n * 31 + B)
    pl = pool(cls, wq, seed)
    rot = rng.randrange(len(pl)) if n < len(pl) + 40 else 0
    inside = [pl[(rot + i) % len(pl)] for i in range(n)]
    # padding lanes: the tail of the last wave and of one inner wave
    pads = set(range(n - 5, n))
    if n >= 3 * WAVE:
        pads |= set(range(2 * WAVE - 3, 2 * WAVE))
    # an invalid key: one whole wave (the key is wave-uniform)
    badwave = 1 if n >= 3 * WAVE else None
    avoid = set(pads) | (set(range(badwave * WAVE, (badwave + 1) * WAVE)) if badwave is not None else set())
    S, spots = chain_spots(n, B, wpb, avoid)
    kinds = ["s=0", "s=n", "s=n+1", "s=ones", "r=0", "r=n", "r=n+1", "r=ones", "status", "pad"]
    ones = (1 << (8 * M.EC_BYTES[cls])) - 1
    val = {"0": 0, "n": M.EC_N[cls], "n+1": M.EC_N[cls] + 1, "ones": ones}
    forced = {}
    for q, (i, j) in enumerate(spots):
        forced[i + j * S] = kinds[q % len(kinds)]
    for q, (i, j) in enumerate(spots):
        for p in range(i, n, S):
            if p in forced:
                continue
            pads.discard(p)                                   # the rejected token's neighbours are valid
            if inside[p].scalars(cls) is None:
                inside[p] = rand_valid(rng, cls, tag="neighbour")
    for p, kind in forced.items():
        t = rand_valid(rng, cls, tag="chain-rej-" + kind)
        pads.discard(p)
        if kind == "pad":
            pads.add(p)
        elif kind == "status":
            t.status = ST_REJECT
        elif kind[0] == "s":
            t.s = val[kind[2:]]
        else:
            t.r = val[kind[2:]]
        inside[p] = t
    slots = [rand_valid(rng, cls, tag="outside") for _ in range(npad)]
    keys = [0] * npad
    for p in range(n):
        t = inside[p]
        if badwave is not None and p // WAVE == badwave:
            keys[begin + p] = 1
            if t is not None:
                t = Tok(t.alg, t.r, t.s, t.digest, t.tag + "/bad-key", t.status, key_ok=False)
        slots[begin + p] = None if p in pads else t
    return slots, keys, set(forced)


def words(v, nw):
    return [(v >> (32 * q)) & 0xFFFFFFFF for q in range(nw)]


def run_case(tk, cls, wq, wpb, B, slots, keys, begin, end, exc_reset=1, exc_in=0x1234567):
    npad = len(slots)
    cw = (M.EC_BYTES[cls] + 3) // 4
    jobs = np.zeros((npad, 4), dtype=np.uint32)
    sigw = np.full((SIG_ROWS, npad), POISON, dtype=np.uint32)
    dig = np.full((DIG_ROWS, npad), POISON, dtype=np.uint32)
    st_in = np.full(npad, ST_POISON, dtype=np.uint8)
    for p, t in enumerate(slots):
        if t is None:
            jobs[p, 3] = keys[p] | (JOB_PAD << 16)
            continue
        jobs[p, 3] = keys[p] | (t.alg << 16)
        # prep writes the alg's words and zeroes up to the curve's
        nw = max(cw, (M.ES_SIZE[t.alg] + 3) // 4)
        assert t.r >> (32 * nw) == 0 and t.s >> (32 * nw) == 0
        sigw[0:nw, p] = words(t.r, nw)
        sigw[EC_S_ROW:EC_S_ROW + nw, p] = words(t.s, nw)
        # digest rows past the words the alg and the curve use stay poison
        hw = min(M.ES_HASH[t.alg], M.EC_BYTES[cls]) // 4
        dig[0:hw, p] = [int.from_bytes(t.digest[4 * q:4 * q + 4], "big") for q in range(hw)]
        if begin <= p < end:
            st_in[p] = t.status
    valid = np.array([1, 0], dtype=np.int32)
    digs = np.zeros((M.ec_digit_rows(cls), npad), dtype=np.uint32)
    st_out = np.zeros(npad, dtype=np.uint8)
    exc = np.zeros(1, dtype=np.uint32)
    rc = tk.tk_ec_scalar(cls, wq, wpb, B, npad, begin, end, jobs.ctypes.data, 2, valid.ctypes.data, sigw.ctypes.data,
                         dig.ctypes.data, st_in.ctypes.data, exc_reset, exc_in, digs.ctypes.data, st_out.ctypes.data,
                         exc.ctypes.data)
    if rc == -2:
        pytest.exit("tk_ec_scalar: HIP error; nothing more is launched on this device", returncode=3)
    assert rc == 0
    return digs.view(np.int32), st_out, st_in, int(exc[0])


def check_case(cls, wq, slots, begin, end, digs, st_out, st_in, must_reject=()):
    wg = M.EC_WG[cls]
    ng, nq = M.ec_windows(cls, wg), M.ec_windows(cls, wq)
    rows = M.ec_digit_rows(cls)
    poison = np.int32(np.uint32(POISON).view(np.int32))
    bad, accepted, rejected = [], 0, 0
    for p, t in enumerate(slots):
        col = [int(x) for x in digs[:, p]]
        if not begin <= p < end:
            if any(x != poison for x in col) or st_out[p] != st_in[p]:
                bad.append((p, "outside the launch, touched"))
            continue
        if t is None:
            if st_out[p] != st_in[p]:
                bad.append((p, "padding lane, status %d" % st_out[p]))
            continue
        want = t.scalars(cls)
        if want is None:
            rejected += 1
            if st_out[p] != ST_REJECT:
                bad.append((p, t.tag, "model rejects, status %d" % st_out[p]))
            continue
        accepted += 1
        if st_out[p] != ST_OK:
            bad.append((p, t.tag, "model accepts, status %d" % st_out[p]))
            continue
        d1, d2 = col[:ng], col[ng:ng + nq]
        if any(not -(1 << (wg - 1)) <= d < (1 << (wg - 1)) for d in d1) or M.digits_value(d1, wg) != want[0]:
            bad.append((p, t.tag, "u1", hex(want[0]), d1))
        if any(not -(1 << (wq - 1)) <= d < (1 << (wq - 1)) for d in d2) or M.digits_value(d2, wq) != want[1]:
            bad.append((p, t.tag, "u2", hex(want[1]), d2))
        if (d1, d2) != (M.recode(want[0], wg, ng, True)[0], M.recode(want[1], wq, nq, True)[0]):
            bad.append((p, t.tag, "digits differ from the model's recoding"))
        if any(x != poison for x in col[ng + nq:rows]):
            bad.append((p, t.tag, "rows past the width's windows written"))
    for p in must_reject:
        t = slots[begin + p]
        assert t is None or t.scalars(cls) is None
    assert not bad, (len(bad), bad[:6])
    return accepted, rejected


# (n, B, wpb): S = ceil(n / B) threads with work
#   320 / 3 : S = 107, threads 106 and above have a shorter chain; one block with 149 idle threads in block_inv
#   1344 / 16 : S = 84;  64 / 16 : four threads of 16 tokens;  640 / 2 : S = 320, two blocks
SHAPES = [(320, 3, 4), (1344, 16, 4), (64, 16, 4), (640, 2, 4), (320, 1, 4), (320, 1, 1), (320, 3, 1)]


def _cases():
    out = []
    for cls in (M.CLS_P256, M.CLS_P384, M.CLS_P521):
        tiers = M.EC_WQ[cls]
        for (n, B, wpb) in SHAPES:
            if wpb == 1:
                ws = [tiers[-1]]                       # WPB = 1 is built at the narrowest width
            elif (n, B) == (320, 3):
                ws = list(tiers)                       # every width
            else:
                ws = [tiers[0], tiers[-1]]
            for wq in ws:
                out.append(pytest.param(cls, wq, n, B, wpb, id="%s-w%d-n%d-B%d-wpb%d" % (NAMES[cls], wq, n, B, wpb)))
    return out


@pytest.mark.parametrize("cls,wq,n,B,wpb", _cases())
def test_ec_scalar_exact(tk, cls, wq, n, B, wpb):
    """begin = 0 with npad = n, then the same tokens at begin = 128 with npad > end"""
    seed = cls * 100 + wq
    for begin, tail in ((0, 0), (128, 64)):
        npad = begin + n + tail
        slots, keys, forced = build_case(cls, wq, n, B, wpb, begin, npad, seed)
        digs, st_out, st_in, exc = run_case(tk, cls, wq, wpb, B, slots, keys, begin, begin + n)
        acc, rej = check_case(cls, wq, slots, begin, begin + n, digs, st_out, st_in, forced)
        assert exc == 0                                # exc_reset = 1
        assert acc >= n // 4 and rej >= min(len(forced), 3)
    # exc_reset = 0: the counter is left alone, everything else the same
    digs2, st2, st_in2, exc = run_case(tk, cls, wq, wpb, B, slots, keys, begin, begin + n, exc_reset=0, exc_in=0x1234567)
    assert exc == 0x1234567
    assert np.array_equal(digs2, digs) and np.array_equal(st2, st_out)


def test_hook_refuses_bad_arguments(tk):
    npad = 128
    buf = np.zeros((SIG_ROWS + DIG_ROWS + 40) * npad, dtype=np.uint32)
    jobs = np.zeros((npad, 4), dtype=np.uint32)
    jobs[:, 3] = M.ES256 << 16

    def call(cls=M.CLS_P256, wq=20, wpb=4, B=1, npad=npad, begin=0, end=64, jobs=jobs, nkeys=2):
        b = buf.ctypes.data
        return tk.tk_ec_scalar(cls, wq, wpb, B, npad, begin, end, jobs.ctypes.data, nkeys, b, b, b, b, 1, 0, b, b, b)

    assert call() == 0
    mixed, badalg, badkey = jobs.copy(), jobs.copy(), jobs.copy()
    mixed[5, 3] |= 1                              # a second key inside a wave
    badalg[70, 3] = 1 << 16                       # RS256
    badkey[64:128, 3] |= 2                        # key 2 of 2
    for kw in (dict(cls=3), dict(cls=7), dict(wq=21), dict(wq=16), dict(wpb=2), dict(wpb=1, wq=26), dict(B=0),
               dict(B=17), dict(npad=100), dict(end=32), dict(end=192), dict(begin=64), dict(begin=-64),
               dict(jobs=mixed), dict(jobs=badalg), dict(jobs=badkey), dict(nkeys=0)):
        assert call(**kw) == -1, kw
