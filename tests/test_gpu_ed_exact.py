"""Exact parity of Ed25519's scalar-level stages (kernels/ed25519.hip) with
big-integer arithmetic (tests/scalar_model.py), through the test hooks of
cap_amd/csrc/tests/tk_ed.hip.  The verify chain shows these stages through the
accept bit only, on SHA-random k, and runs k_ed_finish with one token per
thread below 262,144 padded tokens.

  * tk_ed_scalar: k = H mod L (ed_k_mod_l, shared by k_ed_point,
    k_ed_point_split and k_ed_small) limb for limb at H = 0, 1, L - 1, L, L + 1,
    2L, 2^252, 2^256 - 1, 2^512 - 1, the largest multiple of L below 2^512 and
    its neighbours, and random H; the S verdict (ed_s_ok: S < L and sig[63] &
    0xE0 == 0) around L and with each of the bits 253, 254, 255 set; the signed
    recoding (carry above 2^(W-1): digits in (-2^(W-1), 2^(W-1)]) of k at every
    key-table tier and of S at the base-point width, on chosen window patterns.
  * tk_ed_finish: the production k_ed_finish at B = 1, 2, 3, 16 tokens per
    thread: verdict == (encode(X / Z, Y / Z) == R byte for byte) for random
    projective points with canonical and lazy limbs, Z = 1, x = 0, y = p - 1,
    encodings differing in the sign bit or in bit 0 alone, a non-canonical R;
    rejected tokens and padding lanes at every chain position contribute Z = 1
    (their X, Y, Z rows hold poison), get verdict 0 / no write, and leave
    their neighbours' verdicts exact; nothing outside [begin, end) is touched.
Every assertion is exact equality."""
import ctypes
import os
import random

import numpy as np
import pytest

from tests import scalar_model as M
from tests.test_gpu_ec_scalar_exact import SHAPES, chain_spots

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_OK, ST_REJECT = 0, 1
JOB_PAD, WAVE, ALG_EDDSA = 15, 64, 10
POISON = 0xA5A5A5A5
FE_L = 10
FE_SHIFT = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]     # limb i of radix 2^25.5 sits at bit ceil(25.5 i)
FE_BITS = [26, 25, 26, 25, 26, 25, 26, 25, 26, 25]
P, L = M.ED_P, M.ED_L


@pytest.fixture(scope="module")
def tk():
    lib = ctypes.CDLL(os.path.join(ROOT, "cap_amd", "libcapjwt_tk.so"))
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.tk_ed_scalar.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, vp]
    lib.tk_ed_finish.argtypes = [ctypes.c_int, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp]
    return lib


def _die_on_hip_error(rc, name):
    if rc == -2:
        pytest.exit(name + ": HIP error; nothing more is launched on this device", returncode=3)
    assert rc == 0


# ------------------------------------------------------------------ k, S, digits
ed_patterns = M.ed_patterns          # (tests/scalar_model.py: the CPU model tests use them too)


def test_k_mod_l_s_check_and_recoding(tk):
    rng = random.Random(25519)
    top = (2**512 - 1) // L * L
    hs = [0, 1, L - 1, L, L + 1, 2 * L, 2 * L - 1, 2 * L + 1, 2**252, 2**256 - 1, 2**512 - 1, top - 1, top, top + 1,
          2**511, 2**280, 2**280 - 1, 2**504]
    assert top + 1 < 2**512
    for w in M.ED_WA:
        for u in ed_patterns(w):
            hs += [u, u + rng.randrange((2**512 - u) // L) * L]               # as it is, and behind a real reduction
    hs += [rng.randrange(2**512) for _ in range(500)]
    ss = [0, 1, L - 1, L, L + 1, 2**253 - 1, 2**252, 2**253, 2**254, 2**255, (L - 1) | 2**253, (L - 1) | 2**254,
          (L - 1) | 2**255, 5 | 2**253, 5 | 2**254, 5 | 2**255, 2**256 - 1]
    ss += ed_patterns(M.ED_WB)
    ss += [rng.randrange(L) for _ in range(100)] + [rng.randrange(2**256) for _ in range(100)]
    n = max(len(hs), len(ss))
    hs += [rng.randrange(2**512) for _ in range(n - len(hs))]
    ss += [rng.randrange(L) for _ in range(n - len(ss))]

    dig = np.zeros((16, n), dtype=np.uint32)
    srows = np.zeros((8, n), dtype=np.uint32)
    for i, (h, s) in enumerate(zip(hs, ss)):
        hb = h.to_bytes(64, "little")                                         # the digest bytes; rows are big-endian words
        dig[:, i] = [int.from_bytes(hb[4 * q:4 * q + 4], "big") for q in range(16)]
        srows[:, i] = [(s >> (32 * q)) & 0xFFFFFFFF for q in range(8)]
    krows = sum(M.ed_windows(w) for w in M.ED_WA)
    nb = M.ed_windows(M.ED_WB)
    k = np.zeros((10, n), dtype=np.uint32)
    sok = np.zeros(n, dtype=np.uint8)
    kdig = np.zeros((krows, n), dtype=np.int32)
    sdig = np.zeros((nb, n), dtype=np.int32)
    _die_on_hip_error(tk.tk_ed_scalar(n, dig.ctypes.data, srows.ctypes.data, k.ctypes.data, sok.ctypes.data,
                                      kdig.ctypes.data, sdig.ctypes.data), "tk_ed_scalar")
    bad = []
    for i, (h, s) in enumerate(zip(hs, ss)):
        want = M.ed_k(h.to_bytes(64, "little"))
        assert want == h % L
        limbs = [int(x) for x in k[:, i]]
        if any(x >> 28 for x in limbs) or sum(x << (28 * j) for j, x in enumerate(limbs)) != want:
            bad.append(("k", hex(h), limbs))
        if int(sok[i]) != int(M.ed_s_ok(s.to_bytes(32, "little"))):
            bad.append(("S verdict", hex(s), int(sok[i])))
        row = 0
        for w in M.ED_WA:
            nw = M.ed_windows(w)
            d = [int(x) for x in kdig[row:row + nw, i]]
            row += nw
            ref, carry = M.recode(want, w, nw, False)
            assert carry == 0
            if d != ref or M.digits_value(d, w) != want or any(not -(1 << (w - 1)) < x <= (1 << (w - 1)) for x in d):
                bad.append(("k digits", w, hex(h), d))
        if s < L:
            d = [int(x) for x in sdig[:, i]]
            ref, carry = M.recode(s, M.ED_WB, nb, False)
            assert carry == 0
            if d != ref or M.digits_value(d, M.ED_WB) != s:
                bad.append(("S digits", hex(s), d))
    assert not bad, (len(bad), bad[:5])
    assert tk.tk_ed_scalar(0, dig.ctypes.data, srows.ctypes.data, k.ctypes.data, sok.ctypes.data, kdig.ctypes.data,
                           sdig.ctypes.data) == -1
    assert tk.tk_ed_scalar(n, None, srows.ctypes.data, k.ctypes.data, sok.ctypes.data, kdig.ctypes.data,
                           sdig.ctypes.data) == -1


# ------------------------------------------------------------------ k_ed_finish
def fe_value(limbs):
    return sum(int(x) << s for x, s in zip(limbs, FE_SHIFT))


def fe_canon(v):
    v %= P
    return [(v >> s) & ((1 << b) - 1) for s, b in zip(FE_SHIFT, FE_BITS)]


def fe_lazy(rng):
    return [rng.randrange(1 << 31) for _ in range(FE_L)]


class Pt:
    """one live token: X, Y, Z limbs, the 32 R bytes of its signature, its status"""

    def __init__(self, X, Y, Z, R, tag, status=ST_OK):
        self.X, self.Y, self.Z, self.R, self.tag, self.status = X, Y, Z, R, tag, status

    def verdict(self):
        if self.status != ST_OK:
            return 0
        return int(M.ed_encode(fe_value(self.X), fe_value(self.Y), fe_value(self.Z)) == self.R)


def enc_of(X, Y, Z):
    return M.ed_encode(fe_value(X), fe_value(Y), fe_value(Z))


def flip(b, byte, bit):
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


def rand_point(rng, lazy, tag="rand"):
    while True:
        X, Y, Z = (fe_lazy(rng) for _ in range(3)) if lazy else (fe_canon(rng.randrange(P)) for _ in range(3))
        if fe_value(Z) % P:
            return Pt(X, Y, Z, enc_of(X, Y, Z), tag + ("-lazy" if lazy else "-canon"))


def ed_pool(seed):
    rng = random.Random(seed)
    out = []
    for lazy in (False, True):
        t = rand_point(rng, lazy); t.Z = fe_canon(1); t.R = enc_of(t.X, t.Y, t.Z); t.tag = "Z=1"; out.append(t)
        t = rand_point(rng, lazy); t.R, t.tag = flip(t.R, 31, 7), "rej-sign-bit"; out.append(t)
        t = rand_point(rng, lazy); t.R, t.tag = flip(t.R, 0, 0), "rej-bit0"; out.append(t)
        t = rand_point(rng, lazy); t.R, t.tag = flip(t.R, 31, 6), "rej-bit254"; out.append(t)
        t = rand_point(rng, lazy); t.R, t.tag = flip(t.R, 16, 3), "rej-mid"; out.append(t)
        # x = 0: the sign bit is clear; set, it is rejected
        t = rand_point(rng, lazy); t.X = fe_canon(0); t.R = enc_of(t.X, t.Y, t.Z); t.tag = "x=0"; out.append(t)
        assert t.R[31] >> 7 == 0
        t = rand_point(rng, lazy); t.X = fe_canon(0); t.R = flip(enc_of(t.X, t.Y, t.Z), 31, 7); t.tag = "rej-x=0-sign"
        out.append(t)
        # y = p - 1 and y = 0
        for y in (P - 1, 0, 1):
            t = rand_point(rng, lazy); t.Y = fe_canon(y * fe_value(t.Z)); t.R = enc_of(t.X, t.Y, t.Z)
            t.tag = "y=%d" % (y if y < 2 else -1); out.append(t)
            assert int.from_bytes(t.R, "little") & ((1 << 255) - 1) == y
        # y < 19: R with y + p in its low 255 bits is the same point, not canonical: rejected
        for y in (0, 3, 18):
            t = rand_point(rng, lazy); t.Y = fe_canon(y * fe_value(t.Z))
            good = int.from_bytes(enc_of(t.X, t.Y, t.Z), "little")
            assert (good & ((1 << 255) - 1)) == y and y + P < 1 << 255
            t.R, t.tag = ((good & (1 << 255)) | (y + P)).to_bytes(32, "little"), "rej-noncanonical-R"
            out.append(t)
        # x odd and x even, as chosen values
        for x in (1, 2, P - 1, P - 2):
            t = rand_point(rng, lazy); t.X = fe_canon(x * fe_value(t.Z)); t.R = enc_of(t.X, t.Y, t.Z)
            t.tag = "x=%d" % x; out.append(t)
            assert t.R[31] >> 7 == x & 1
        t = rand_point(rng, lazy); t.status, t.tag = ST_REJECT, "rej-status"; out.append(t)
    for i in range(120):
        out.append(rand_point(rng, i % 2 == 1))
    assert {t.verdict() for t in out} == {0, 1}
    return out


def build_finish_case(n, B, wpb, begin, npad, seed):
    rng = random.Random(seed * 7919 + n * 31 + B)
    pl = ed_pool(seed)
    rot = rng.randrange(len(pl)) if n < len(pl) else 0
    inside = [pl[(rot + i) % len(pl)] for i in range(n)]
    pads = set(range(n - 5, n))
    if n >= 3 * WAVE:
        pads |= set(range(2 * WAVE - 3, 2 * WAVE))
    S, spots = chain_spots(n, B, wpb, set(pads))
    forced = {i + j * S: ("status", "pad")[q % 2] for q, (i, j) in enumerate(spots)}
    for i, j in spots:
        for p in range(i, n, S):
            if p not in forced:
                pads.discard(p)                               # the non-OK token's neighbours are live and ST_OK
                if inside[p].status != ST_OK:
                    inside[p] = rand_point(rng, p % 2 == 1, "neighbour")
    for p, kind in forced.items():
        pads.discard(p)
        if kind == "pad":
            pads.add(p)
        else:
            t = rand_point(rng, True, "chain-rej")
            t.status = ST_REJECT
            inside[p] = t
    slots = [rand_point(rng, True, "outside") for _ in range(npad)]
    for p in range(n):
        slots[begin + p] = None if p in pads else inside[p]
    return slots


def run_finish(tk, B, slots, begin, end):
    npad = len(slots)
    jobs = np.zeros((npad, 4), dtype=np.uint32)
    st_in = np.zeros(npad, dtype=np.uint8)
    xyz = np.full((3 * FE_L, npad), POISON, dtype=np.uint32)
    rrows = np.full((8, npad), POISON, dtype=np.uint32)
    for p, t in enumerate(slots):
        if t is None:
            jobs[p, 3] = JOB_PAD << 16
            st_in[p] = 0xA5
            continue
        jobs[p, 3] = (ALG_EDDSA << 16) | (86 << 20)
        st_in[p] = t.status
        rrows[:, p] = [int.from_bytes(t.R[4 * q:4 * q + 4], "little") for q in range(8)]
        if t.status == ST_OK:                                 # a rejected token's X, Y, Z stay poison: never read
            xyz[:, p] = t.X + t.Y + t.Z
    verdict = np.zeros(npad, dtype=np.uint8)
    xyz_out = np.zeros((4 * FE_L, npad), dtype=np.uint32)
    st_out = np.zeros(npad, dtype=np.uint8)
    _die_on_hip_error(tk.tk_ed_finish(B, npad, begin, end, jobs.ctypes.data, st_in.ctypes.data, xyz.ctypes.data,
                                      rrows.ctypes.data, verdict.ctypes.data, xyz_out.ctypes.data,
                                      st_out.ctypes.data), "tk_ed_finish")
    return verdict, xyz_out, st_out, st_in, xyz


@pytest.mark.parametrize("n,B", sorted({(n, B) for n, B, wpb in SHAPES}))
def test_ed_finish_exact(tk, n, B):
    """begin = 0 with npad = n, then begin = 128 with npad > end (k_ed_finish always runs four waves per block)"""
    for begin, tail in ((0, 0), (128, 64)):
        npad, end = begin + n + tail, begin + n
        slots = build_finish_case(n, B, 4, begin, npad, 77)
        verdict, xyz_out, st_out, st_in, xyz_in = run_finish(tk, B, slots, begin, end)
        bad, seen = [], {0: 0, 1: 0}
        for p, t in enumerate(slots):
            if not begin <= p < end:
                if verdict[p] != 0xA5 or any(int(x) != POISON for x in xyz_out[3 * FE_L:, p]):
                    bad.append((p, "outside the launch, touched"))
            elif t is None:
                if verdict[p] != 0xA5:
                    bad.append((p, "padding lane, verdict written", int(verdict[p])))
            else:
                seen[t.verdict()] += 1
                if int(verdict[p]) != t.verdict():
                    bad.append((p, t.tag, "verdict", int(verdict[p]), "want", t.verdict()))
        assert not bad, (len(bad), bad[:8])
        assert np.array_equal(xyz_out[:3 * FE_L], xyz_in)     # X, Y, Z are inputs only
        assert np.array_equal(st_out, st_in)
        assert seen[1] >= n // 4 and seen[0] >= 3


def test_ed_finish_hook_refuses_bad_arguments(tk):
    slots = build_finish_case(64, 1, 4, 0, 128, 5)
    npad = len(slots)
    jobs = np.zeros((npad, 4), dtype=np.uint32)
    jobs[:, 3] = ALG_EDDSA << 16
    z8 = np.zeros(npad, dtype=np.uint8)
    buf = np.zeros((40, npad), dtype=np.uint32)
    buf[2 * FE_L] = 1                                         # Z = 1

    o_verdict, o_xyz, o_status = z8.copy(), buf.copy(), z8.copy()

    def call(B=1, npad=npad, begin=0, end=64, xyz=buf):
        return tk.tk_ed_finish(B, npad, begin, end, jobs.ctypes.data, z8.ctypes.data, xyz.ctypes.data, buf.ctypes.data,
                               o_verdict.ctypes.data, o_xyz.ctypes.data, o_status.ctypes.data)

    assert call() == 0
    big = buf.copy()
    big[7, 9] = 1 << 31                                       # a limb fe_to_mont does not accept
    for kw in (dict(B=0), dict(B=17), dict(npad=100), dict(end=32), dict(end=192), dict(begin=64), dict(begin=-64),
               dict(xyz=big)):
        assert call(**kw) == -1, kw
