"""Exact parity of the prep stage (kernels/prep.hip k_prep_mid + k_prep, through
the production launch_prep) with hashlib and base64, word for word, through the
test hook tk_prep (cap_amd/csrc/tests/tk_prep.hip).  The verify chain only shows
accept / reject, at the token lengths the fixtures happen to have; here

  * the digest of every signing-input length 1..300 and around the 128-byte
    window edges 384 / 512 / 640, at every arena alignment, packed back to back
    (a read past `len` meets a neighbour's bytes), for the RSA and EC variants
    at hash masks 1 / 2 / 3 (algs mixed inside a wave) and Ed25519's
    SHA-512(R || A || M), in three job orders: by length, shuffled (window
    counts mixed inside a wave), and with ragged waves (one live lane at lane 0,
    one at lane 63, 63 live lanes);
  * the shared-block-0 midstate (k_prep_mid): sharing runs, a differing lane, a
    differing first token, first tokens of one block / with the pad byte inside
    the recorded block, waves mixing one-block lanes with sharing lanes --
    digests stay exact and the recorded block, midstate and flag of every run
    are as specified (that a wave then starts from the midstate is not visible);
  * the base64url decode into the three row layouts: status, decoded length and
    every row the class's arithmetic kernel reads (rows are poisoned with
    0xA5A5A5A5 before the launch, so a missed zeroing shows), for short, odd,
    standard and over-long character counts, every segment alignment, the
    word-wise and the byte-serial path, bad characters at the window edges, and
    every RSA limb layout.
Every assertion is exact equality."""
import base64
import collections
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS_RSA2K, CLS_RSA3K, CLS_RSA4K, CLS_P256, CLS_P384, CLS_P521, CLS_ED25519 = 1, 2, 3, 4, 5, 6, 7
ST_OK, ST_REJECT = 0, 1
JOB_PAD, WAVE, SIGW_ROWS, DIG_ROWS, EC_S_ROW = 15, 64, 520, 16, 32
POISON = 0xA5A5A5A5
ALG_EDDSA = 10
B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
ES_SIZE = {7: 32, 8: 48, 9: 66}

Job = collections.namedtuple("Job", "off ln soff nch alg msg sig tag")
Result = collections.namedtuple("Result", "dig sigw status siglen zrows ec_words mid")
PREP_MID_WORDS = 32


def alg_hash(alg):
    return hashlib.sha256 if alg in (1, 4, 7) else hashlib.sha384 if alg in (2, 5, 8) else hashlib.sha512


@pytest.fixture(scope="module")
def tk():
    L = ctypes.CDLL(os.path.join(ROOT, "cap_amd", "libcapjwt_tk.so"))
    vp = ctypes.c_void_p
    L.tk_prep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_uint64, vp, ctypes.c_int64,
                          ctypes.c_int, vp, vp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_int),
                          ctypes.POINTER(ctypes.c_int), vp]
    L.tk_prep.restype = ctypes.c_int
    return L


class Arena:
    """token bytes packed back to back; at most 3 non-zero filler bytes put a string at its alignment"""

    def __init__(self, seed):
        self.buf = bytearray()
        self.rng = random.Random(seed)

    def put(self, data, align):
        while len(self.buf) % 4 != align % 4:
            self.buf.append(self.rng.randrange(1, 256))
        off = len(self.buf)
        self.buf += data
        return off

    def job(self, msg, sig, alg, align, sig_align=None, tag=None):
        off = self.put(msg, align)
        soff = self.put(sig, (align + 1) if sig_align is None else sig_align)
        return Job(off, len(msg), soff, len(sig), alg, bytes(msg), bytes(sig), tag)


def layout(runs):
    """[(key, [Job or None, ..]), ..] -> padded slots [(key, Job or None)]: every
    key run filled up to whole waves with padding lanes (None)"""
    slots = []
    for key, jobs in runs:
        jobs = list(jobs) + [None] * (-len(jobs) % WAVE)
        slots += [(key, j) for j in jobs]
    return slots


def call_prep(tk, cls, hash_mask, use_mid, buf, rec, nkeys, nlimbs=None, pubs=None):
    n = len(rec)
    buf = np.frombuffer(bytes(buf), dtype=np.uint8)
    nl = np.array(nlimbs if nlimbs is not None else [0] * nkeys, dtype=np.uint32)
    pb = np.frombuffer(b"".join(pubs) if pubs is not None else bytes(32 * nkeys), dtype=np.uint8)
    dig = np.zeros((DIG_ROWS, max(n, 1)), dtype=np.uint32)
    sigw = np.zeros((SIGW_ROWS, max(n, 1)), dtype=np.uint32)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    siglen = np.zeros(max(n, 1), dtype=np.uint16)
    mid = np.zeros((max(nkeys, 1), PREP_MID_WORDS), dtype=np.uint32)
    zr, ew = ctypes.c_int(), ctypes.c_int()
    rec = np.ascontiguousarray(rec, dtype=np.uint32)
    rc = tk.tk_prep(cls, hash_mask, use_mid, buf.ctypes.data, len(buf), rec.ctypes.data, n, nkeys, nl.ctypes.data,
                    pb.ctypes.data, dig.ctypes.data, sigw.ctypes.data, status.ctypes.data, siglen.ctypes.data,
                    ctypes.byref(zr), ctypes.byref(ew), mid.ctypes.data)
    return rc, Result(dig, sigw, status, siglen, zr.value, ew.value, mid)


def records(slots):
    rec = np.zeros((len(slots), 4), dtype=np.uint32)
    for p, (key, j) in enumerate(slots):
        if j is None:
            rec[p] = (0, 0, 0, key | (JOB_PAD << 16))
        else:
            rec[p] = (j.off, j.ln, j.soff, key | (j.alg << 16) | (j.nch << 20))
    return rec


def run_prep(tk, cls, hash_mask, use_mid, buf, slots, nkeys, nlimbs=None, pubs=None):
    rc, res = call_prep(tk, cls, hash_mask, use_mid, buf, records(slots), nkeys, nlimbs, pubs)
    if rc == -2:
        pytest.exit("tk_prep: HIP error; nothing more is launched on this device", returncode=3)
    assert rc == 0
    return res


def b64dec(chars):
    return base64.urlsafe_b64decode(bytes(chars) + b"=" * (-len(chars) % 4))


def check_digests(res, slots, pubs=None):
    """every live slot's digest rows == hashlib; padding lanes wrote nothing"""
    bad, live = [], 0
    for p, (key, j) in enumerate(slots):
        if j is None:
            assert res.status[p] == ST_REJECT
            assert (res.dig[:, p] == POISON).all() and (res.sigw[:, p] == POISON).all(), p
            continue
        live += 1
        m = j.msg if j.alg != ALG_EDDSA else b64dec(j.sig)[:32] + pubs[key] + j.msg
        d = alg_hash(j.alg)(m).digest()
        exp = np.frombuffer(d, dtype=">u4").astype(np.uint32)
        got = res.dig[:len(exp), p]
        if not (got == exp).all():
            bad.append("wrong digest: len=%d off%%4=%d alg=%d slot=%d tag=%s got=%08x.. want=%08x.." %
                       (j.ln, j.off % 4, j.alg, p, j.tag, got[0], exp[0]))
    assert not bad, (len(bad), bad[:8])
    return live


# ---------------------------------------------------------------- digests
LENS = sorted(set(range(1, 301)) | {128 * m + d for m in (3, 4, 5) for d in range(-9, 9)})
RSA_ALGS = {1: [1, 4], 2: [2, 3, 5, 6], 3: [1, 2, 3, 4, 5, 6]}
EC_ALGS = {1: [7], 2: [8, 9], 3: [7, 8, 9]}


def digest_jobs(seed, algs, sig_bytes_of):
    """one job per (length, alignment); a signature of the alg's proper size each"""
    ar = Arena(seed)
    rng = ar.rng
    jobs = []
    for ln in LENS:
        for al in range(4):
            alg = algs[(ln + al) % len(algs)]
            msg = rng.randbytes(ln)
            sig = base64.urlsafe_b64encode(rng.randbytes(sig_bytes_of(alg))).rstrip(b"=")
            jobs.append(ar.job(msg, sig, alg, al))
    return ar, jobs


def orders(jobs, seed, nkeys=1):
    """the three job orders, each as key runs [(key, [Job or None])]"""
    def split(seq):
        per = (len(seq) + nkeys - 1) // nkeys
        return [(k, seq[k * per:(k + 1) * per]) for k in range(nkeys)]
    by_len = sorted(jobs, key=lambda j: (j.ln, j.off))
    sh = list(jobs)
    random.Random(seed).shuffle(sh)
    # ragged: whole waves, then 63 live lanes + 1 pad, a lone lane 0, a lone lane 63, and a short tail
    body = len(sh) - 63 - 2 - 7
    body -= body % WAVE
    rag = sh[:body] + sh[body:body + 63] + [None] + [sh[body + 63]] + [None] * 63 + [None] * 63 + [sh[body + 64]]
    rag += sh[body + 65:]
    assert sum(j is not None for j in rag) == len(jobs)
    out = {"by-length": split(by_len), "shuffled": split(sh)}
    if nkeys == 1:
        out["ragged"] = [(0, rag)]
    else:                       # the ragged waves under the last key, the whole waves spread over the others
        per = (body // WAVE + nkeys - 2) // (nkeys - 1) * WAVE
        out["ragged"] = [(k, rag[k * per:min((k + 1) * per, body)]) for k in range(nkeys - 1)] + \
            [(nkeys - 1, rag[body:])]
    return out


@pytest.mark.parametrize("hash_mask", [1, 2, 3])
def test_digest_rsa_prep(tk, hash_mask):
    ar, jobs = digest_jobs(100 + hash_mask, RSA_ALGS[hash_mask], lambda alg: 256)
    assert len(jobs) == 4 * len(LENS) == 1416
    for name, runs in orders(jobs, hash_mask).items():
        slots = layout(runs)
        res = run_prep(tk, CLS_RSA2K, hash_mask, 0, ar.buf, slots, 1, nlimbs=[74])
        assert check_digests(res, slots) == len(jobs), name


@pytest.mark.parametrize("hash_mask", [1, 2, 3])
def test_digest_ec_prep(tk, hash_mask):
    cls = {1: CLS_P256, 2: CLS_P384, 3: CLS_P521}[hash_mask]
    ar, jobs = digest_jobs(200 + hash_mask, EC_ALGS[hash_mask], lambda alg: 2 * ES_SIZE[alg])
    for name, runs in orders(jobs, 10 + hash_mask).items():
        slots = layout(runs)
        res = run_prep(tk, cls, hash_mask, 0, ar.buf, slots, 1)
        assert check_digests(res, slots) == len(jobs), name


def test_digest_ed25519_prep(tk):
    """SHA-512(R || A || M): the 64-byte register prefix, window c >= 1 at
    message word 32c - 16; three keys (A differs by key run)"""
    ar, jobs = digest_jobs(300, [ALG_EDDSA], lambda alg: 64)
    rng = random.Random(301)
    pubs = [rng.randbytes(32) for _ in range(3)]
    for name, runs in orders(jobs, 20, nkeys=3).items():
        slots = layout(runs)
        assert {k for k, j in slots if j is not None} == {0, 1, 2}
        res = run_prep(tk, CLS_ED25519, 2, 0, ar.buf, slots, 3, pubs=pubs)
        assert check_digests(res, slots, pubs) == len(jobs), name
        live = [p for p, (k, j) in enumerate(slots) if j is not None]
        assert (res.status[live] == ST_OK).all() and (res.siglen[live] == 64).all()


# ---------------------------------------------------------------- shared block 0
SHA256_K = [int((p ** (1 / 3) % 1) * 2 ** 32) for p in
            [q for q in range(2, 312) if all(q % d for d in range(2, int(q ** 0.5) + 1))][:64]]
SHA256_H0 = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def sha256_block0(block):
    """SHA-256 state after one 64-byte block from the initial state (FIPS 180-4 6.2.2)"""
    M = 0xffffffff
    rr = lambda x, n: ((x >> n) | (x << (32 - n))) & M        # noqa: E731
    w = [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(16)]
    for i in range(16, 64):
        s0 = rr(w[i - 15], 7) ^ rr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = rr(w[i - 2], 17) ^ rr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & M)
    a, b, c, d, e, f, g, h = SHA256_H0
    for i in range(64):
        t1 = (h + (rr(e, 6) ^ rr(e, 11) ^ rr(e, 25)) + ((e & f) ^ (~e & M & g)) + SHA256_K[i] + w[i]) & M
        t2 = ((rr(a, 2) ^ rr(a, 13) ^ rr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M
        a, b, c, d, e, f, g, h = (t1 + t2) & M, a, b, c, (d + t1) & M, e, f, g
    return [(x + y) & M for x, y in zip(SHA256_H0, (a, b, c, d, e, f, g, h))]


def check_mid_slots(res, runs):
    """what k_prep_mid recorded per key run: the first token's padded block 0, its
    midstate and the valid flag -- or flag 0 when that token is a single block.
    (Whether k_prep then starts a wave from the midstate cannot be seen from
    outside: the digests are the same either way, which is the point.)"""
    recorded = 0
    for key, jobs in runs:
        j, slot = jobs[0], res.mid[key]
        if (j.ln + 9 + 63) // 64 < 2:
            assert slot[24] == 0, key
            continue
        block = (j.msg + b"\x80" + bytes(64))[:64]
        assert slot[24] == 1, key
        assert list(slot[:16]) == [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(16)], key
        assert list(slot[16:24]) == sha256_block0(block), key
        recorded += 1
    return recorded


def mid_runs(seed, algs):
    """key runs for the k_prep_mid scenarios; `algs` cycles over the lanes"""
    ar = Arena(seed)
    rng = ar.rng
    rb = rng.randbytes
    sig = base64.urlsafe_b64encode(rb(256)).rstrip(b"=")
    cnt = [0]

    def J(msg, tag, alg=None):
        cnt[0] += 1
        return ar.job(msg, sig, algs[cnt[0] % len(algs)] if alg is None else alg, cnt[0] % 4, tag=tag)

    def tail():
        return rb(rng.choice([0, 1, 7, 8, 55, 56, 63, 64, 65, 100, 191, 192, 193]))

    a256 = algs[0]
    runs = []
    pre = rb(64)
    runs.append([J(pre + tail(), "shared", a256)] + [J(pre + tail(), "shared") for _ in range(191)])   # 3 waves
    pre = rb(64)
    k1 = [J(pre + tail(), "one-differs", a256)] + [J(pre + tail(), "one-differs") for _ in range(127)]
    odd = bytearray(pre)
    odd[37] ^= 0x10
    k1[70] = J(bytes(odd) + tail(), "the-differing-lane", a256)
    runs.append(k1)
    pre = rb(64)
    odd = bytearray(pre)
    odd[63] ^= 0x01
    runs.append([J(bytes(odd) + tail(), "first-differs", a256)] + [J(pre + tail(), "first-differs") for _ in range(127)])
    pre = rb(64)
    runs.append([J(pre[:40], "first-is-one-block", a256)] + [J(pre + tail(), "after-one-block") for _ in range(127)])
    # first token of 56..63 bytes: the recorded block holds its pad byte; longer tokens share the
    # message bytes, and a whole wave of them has 80 00 .. in the same place (an equal block 0)
    for ln in (56, 60, 63):
        pre = rb(ln)
        k = [J(pre, "first-has-pad-in-block", a256)] + [J(pre + rb(64 - ln) + tail(), "shares-bytes") for _ in range(63)]
        k += [J(pre + b"\x80" + bytes(63 - ln) + tail(), "equals-padded-block", a256) for _ in range(64)]
        runs.append(k)
    pre = rb(64)
    k = [J(pre + tail(), "mixed", a256)]
    for i in range(1, 128):
        k.append(J(pre[:rng.randrange(1, 56)], "mixed-one-block") if i % 3 == 0 else J(pre + tail(), "mixed"))
    runs.append(k)
    return ar, [(key, jobs) for key, jobs in enumerate(runs)]


@pytest.mark.parametrize("cls,hash_mask,algs", [(CLS_RSA2K, 1, [1, 4]), (CLS_RSA2K, 3, [1, 3, 4, 6, 2]),
                                                (CLS_P256, 1, [7]), (CLS_P521, 3, [7, 9, 8])])
def test_midstate_digests(tk, cls, hash_mask, algs):
    ar, runs = mid_runs(400 + cls + hash_mask, algs)
    # every job carries a 256-byte signature (an EC class turns it away; the digest is written all the same)
    slots = layout(runs)
    assert len(slots) // WAVE >= 3 and len(runs) == 8
    nl = [74] * len(runs) if cls == CLS_RSA2K else None
    res = run_prep(tk, cls, hash_mask, 1, ar.buf, slots, len(runs), nlimbs=nl)
    check_digests(res, slots)
    assert check_mid_slots(res, runs) == 7          # every run but the one that opens with a one-block token
    # the same launch without the midstate scratch: identical digests
    ref = run_prep(tk, cls, hash_mask, 0, ar.buf, slots, len(runs), nlimbs=nl)
    live = [p for p, (k, j) in enumerate(slots) if j is not None]
    assert (res.dig[:8, live] == ref.dig[:8, live]).all()


# ---------------------------------------------------------------- signature decode
BAD_CHARS = b"=+/\x7f"
BAD_POS = [0, 127, 128, 129, 255, 256, -1]


def rsa_read_rows(zrows, nlimbs):
    return min(zrows, (28 * nlimbs - 1) // 32 + 2)


def expect_decode(cls, zrows, ec_words, nlimbs, j):
    """(status, siglen, {row: word}) of a job by base64 + the layout rule.  A
    signature the length rules turn away has siglen 0; one turned away for a
    character keeps its decoded length.  Rows are given for ST_OK only."""
    n = j.nch
    if n % 4 == 1:
        return ST_REJECT, 0, None
    D = n // 4 * 3 + (0, 0, 1, 2)[n % 4]
    if D > 4 * zrows:
        return ST_REJECT, 0, None
    if CLS_P256 <= cls <= CLS_P521:
        ks = ES_SIZE.get(j.alg, 0)
        if ks == 0 or D != 2 * ks:
            return ST_REJECT, 0, None
    if any(c not in B64 for c in j.sig):
        return ST_REJECT, D, None
    raw = b64dec(j.sig)
    assert len(raw) == D
    rows = {}
    if cls <= CLS_RSA4K:                                  # LAY_BE: row q = LE word q of the big-endian integer
        v = int.from_bytes(raw, "big")
        for q in range(rsa_read_rows(zrows, nlimbs)):
            rows[q] = (v >> (32 * q)) & 0xffffffff
    elif cls <= CLS_P521:                                 # LAY_SPLIT_BE: r at rows 0.., s at rows EC_S_ROW..
        r, s = int.from_bytes(raw[:ks], "big"), int.from_bytes(raw[ks:], "big")
        for q in range(ec_words):
            rows[q] = (r >> (32 * q)) & 0xffffffff
            rows[EC_S_ROW + q] = (s >> (32 * q)) & 0xffffffff
    else:                                                 # LAY_LE: the bytes as LE words
        v = int.from_bytes(raw, "little")
        for q in range(zrows):
            rows[q] = (v >> (32 * q)) & 0xffffffff
    return ST_OK, D, rows


def check_decode(res, slots, cls, nlimbs):
    bad, n_ok, n_rej = [], 0, 0
    for p, (key, j) in enumerate(slots):
        if j is None:
            assert res.status[p] == ST_REJECT and (res.sigw[:, p] == POISON).all()
            continue
        st, ln, rows = expect_decode(cls, res.zrows, res.ec_words, nlimbs[key] if nlimbs else 0, j)
        got = (int(res.status[p]), int(res.siglen[p]))
        if got != (st, ln):
            bad.append("status/siglen %s, want %s: chars=%d sig_off%%4=%d alg=%d tag=%s" %
                       (got, (st, ln), j.nch, j.soff % 4, j.alg, j.tag))
            continue
        n_ok += st == ST_OK
        n_rej += st != ST_OK
        if rows is not None:
            wrong = [(q, int(res.sigw[q, p]), w) for q, w in rows.items() if int(res.sigw[q, p]) != w]
            if wrong:
                bad.append("wrong rows %s: chars=%d sig_off%%4=%d alg=%d key=%d tag=%s" %
                           ([(q, hex(a), hex(b)) for q, a, b in wrong[:4]], j.nch, j.soff % 4, j.alg, key, j.tag))
        assert (res.sigw[res.zrows:, p] == POISON).all(), j     # nothing is written past the rows the launch covers
    assert not bad, (len(bad), bad[:8])
    return n_ok, n_rej


def decode_jobs(seed, counts, algs, bad_counts):
    """a job per (character count, segment alignment, alg), plus the bad-character jobs"""
    ar = Arena(seed)
    rng = ar.rng
    msg = b"signing.input"
    jobs = []
    for n in counts:
        for al in range(4):
            for alg in algs:
                chars = bytes(rng.choice(B64) for _ in range(n))
                jobs.append(ar.job(msg, chars, alg, (al + n) % 4, sig_align=al, tag="count"))
    for n, alg in bad_counts:
        for pos in sorted({q if q >= 0 else n - 1 for q in BAD_POS if q < n}):
            for ci, c in enumerate(BAD_CHARS):
                chars = bytearray(rng.choice(B64) for _ in range(n))
                chars[pos] = c
                jobs.append(ar.job(msg, bytes(chars), alg, ci, sig_align=(pos + ci) % 4, tag="bad%02x@%d" % (c, pos)))
    return ar, jobs


def chars_for_bytes(d):
    return d // 3 * 4 + (0, 2, 3)[d % 3]


BASE_COUNTS = [2, 3, 4, 6, 7, 8, 5, 9, 42, 43, 44, 85, 86, 87, 127, 128, 129, 175, 176, 177, 341, 342, 343,
               511, 512, 513, 682, 683, 684]


def edge_counts(zrows):
    """just below, at, and just above 4 * zrows decoded bytes (the last must reject)"""
    return [chars_for_bytes(4 * zrows - 1), chars_for_bytes(4 * zrows), chars_for_bytes(4 * zrows + 1)]


@pytest.mark.parametrize("cls,nlimbs", [(CLS_RSA2K, [74]), (CLS_RSA3K, [112]), (CLS_RSA4K, [148]),
                                        (CLS_RSA4K, [148, 296, 592]), (CLS_RSA4K, [296])])
def test_decode_rsa_layout(tk, cls, nlimbs):
    zrows = max((28 * nl - 1) // 32 + 2 for nl in nlimbs)
    counts = sorted(set(BASE_COUNTS + edge_counts(zrows) + [c for nl in nlimbs for c in edge_counts((28 * nl - 1) // 32 + 2)]))
    ar, jobs = decode_jobs(500 + sum(nlimbs), counts, [1, 6], [(342, 1), (343, 1)])
    random.Random(7).shuffle(jobs)
    per = (len(jobs) + len(nlimbs) - 1) // len(nlimbs)
    slots = layout([(k, jobs[k * per:(k + 1) * per]) for k in range(len(nlimbs))])
    res = run_prep(tk, cls, 3, 0, ar.buf, slots, len(nlimbs), nlimbs=nlimbs)
    assert res.zrows == zrows <= SIGW_ROWS
    n_ok, n_rej = check_decode(res, slots, cls, nlimbs)
    assert n_ok >= 100 and n_rej >= 100


@pytest.mark.parametrize("cls", [CLS_P256, CLS_P384, CLS_P521])
def test_decode_ecdsa_layout(tk, cls):
    ar, jobs = decode_jobs(600 + cls, sorted(set(BASE_COUNTS + edge_counts(EC_S_ROW + 17))), [7, 8, 9],
                           [(86, 7), (128, 8), (176, 9)])
    random.Random(8).shuffle(jobs)
    slots = layout([(0, jobs)])
    res = run_prep(tk, cls, 3, 0, ar.buf, slots, 1)
    assert res.zrows == EC_S_ROW + 17 and res.ec_words == {CLS_P256: 8, CLS_P384: 12, CLS_P521: 17}[cls]
    n_ok, n_rej = check_decode(res, slots, cls, None)
    assert n_ok == 12 and n_rej >= 300          # 86 / 128 / 176 characters under ES256 / ES384 / ES512, 4 alignments


def test_decode_ed25519_layout(tk):
    ar, jobs = decode_jobs(700, sorted(set(BASE_COUNTS + edge_counts(16))), [ALG_EDDSA], [(86, ALG_EDDSA), (84, ALG_EDDSA)])
    random.Random(9).shuffle(jobs)
    slots = layout([(0, jobs[:100]), (1, jobs[100:])])
    pubs = [bytes(range(32)), bytes(range(32, 64))]
    res = run_prep(tk, CLS_ED25519, 2, 0, ar.buf, slots, 2, pubs=pubs)
    assert res.zrows == 16
    n_ok, n_rej = check_decode(res, slots, CLS_ED25519, None)
    assert n_ok >= 40 and n_rej >= 60
    # R || A || M is hashed for every signature that has all of R, whatever its length
    ok = [(p, k, j) for p, (k, j) in enumerate(slots) if j is not None and res.status[p] == ST_OK and j.nch >= 43]
    for p, k, j in ok:
        d = hashlib.sha512(b64dec(j.sig)[:32] + pubs[k] + j.msg).digest()
        assert (res.dig[:, p] == np.frombuffer(d, dtype=">u4")).all(), j


# ---------------------------------------------------------------- the hook's own argument checks
def test_hook_refuses_bad_arguments(tk):
    """every malformed launch returns -1 before anything reaches the device"""
    ar = Arena(1)
    j = ar.job(b"abc.def", b"QUJD", 1, 0)
    good = records(layout([(0, [j])]))
    assert call_prep(tk, CLS_RSA2K, 1, 0, ar.buf, good, 1, nlimbs=[74])[0] == 0

    def rc(cls=CLS_RSA2K, hm=1, rec=good, nkeys=1, nlimbs=(74,), buf=ar.buf):
        return call_prep(tk, cls, hm, 0, buf, rec, nkeys, nlimbs=list(nlimbs))[0]

    assert rc(cls=0) == -1 and rc(cls=8) == -1 and rc(hm=0) == -1 and rc(hm=4) == -1
    assert rc(rec=good[:63]) == -1 and rc(rec=good[:0]) == -1            # not whole waves
    assert rc(nlimbs=(75,)) == -1 and rc(cls=CLS_RSA3K) == -1             # limbs the class has no layout for
    assert rc(hm=2) == -1                                                  # RS256 in a SHA-384/512-only launch
    for col, v in ((0, len(ar.buf)), (1, len(ar.buf) + 1), (2, len(ar.buf) - 3)):
        r = good.copy()
        r[0, col] = v                                                      # off + len / sig_off + chars past the arena
        assert rc(rec=r) == -1
    r = good.copy()
    r[5, 3] = 1 | (JOB_PAD << 16)                                         # another key inside the wave
    assert rc(rec=r, nkeys=2, nlimbs=(74, 74)) == -1
    r = good.copy()
    r[0, 3] = 3 | (1 << 16) | (4 << 20)                                   # key index past the key list
    assert rc(rec=r) == -1
    r = good.copy()
    r[9, 0] = 4                                                            # a padding lane with an offset
    assert rc(rec=r) == -1
