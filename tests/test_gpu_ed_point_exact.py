"""Exact parity of the Ed25519 point kernels (kernels/ed25519.hip k_ed_point,
k_ed_point_pf, k_ed_point_split<WA, ED_SPLIT>) with the bit-exact chain model
(tests/ed_point_model.py, held to big integers by tests/test_ed_point_model.py),
through the hook tk_ed_point (cap_amd/csrc/tests/tk_ed_point.hpp).  The verify
chain shows R' = [S]B + [k](-A) only as an accept bit and only for
k = SHA-512(R || A || M) mod L; here H = k + m L is chosen, so k is.

The hook runs the production kernels on SPARSE tables: full geometry, filled
with the poison word, holding only the entries the accepted tokens' digits
name (zero digits name none: the entry that k_ed_point_pf loads for a zero
digit is poison unless a digit names it).  A kernel that reads any other
entry, or adds an entry it should skip, computes on poison and the compare
fails.

One case per key-table tier, one hook call of npad = 256, [64, 192): group 1
on key 0 (A = a B, a known), group 2 on key 1, a key of order 8, at W <= 20 and
on key 0 at W = 22, 24 (two 11.8 GB regions at most).  Tokens: see
ed_point_model.tokens, plus the rejected ones (S = L, L + 1, bit 253 / 254 / 255
of S, siglen 63 / 65, status_in = ST_REJECT) and padding lanes at lane 0, lane
63 and between live tokens of a split wave.  Further calls: at W <= 20 the same
tokens with key 1 invalid (group 2 rejects, group 1 stays exact); at W = 24 and
16 keys with A = B and A = -B and S = k (every window pair cancels / adds the
same point twice; at W = 24 one key per call).

Assertions, all integer equality: forms 0 and 1 (k_ed_point, k_ed_point_pf)
equal chain_one_lane limb for limb, form 2 equals chain_split(ED_SPLIT); each
is [S]B + [k](-A) by big integers with Z != 0; limbs are normalized; status
stays ST_OK.  S = k = 0 leaves the one-lane forms at exactly X = 0, Y = Z = 1;
the split adds neutral elements with add_ext, whose E = B - A is 2p limb by
limb, and ends on X = p's limbs, Y = Z (the model says which).  Rejected tokens
end ST_REJECT in every form (their X, Y, Z are not asserted: k_ed_finish
substitutes Z = 1).  Padding lanes and every slot outside [begin, end) keep
poison X, Y, Z and their status.

Each call prints its model, hook and compare wall times (pytest -s)."""
import ctypes
import os
import random
import time

import numpy as np
import pytest

from tests import ed_point_model as E
from tests import scalar_model as M
from tests import table_model as T
from tests.test_ed_point_model import SECRET, neg, order8_point
from tests.test_gpu_ed_exact import ALG_EDDSA, JOB_PAD, POISON, ST_OK, ST_REJECT, WAVE, _die_on_hip_error, ed_patterns

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPAD, BEGIN, END = 256, 64, 192
ED_SPLIT = 4                                       # kernels/point_form.hpp JG_ED_SPLIT_LANES (the tk fixture asserts it)
P, L = E.P, E.L
PADS = (0, 17, 63, 64 + 30, 127)                   # offsets from BEGIN: lane 0, lane 63, inside split waves
NEUTRAL_XYZ = E.neutral()[:3]
# Random (S, k) pairs per group.  Measured on an MI355X host, one pytest process: with every free lane random (113
# exact tokens a call) the W = 24 case took 1.31 s -- model 0.52 s, compare 0.17 s, hook 0.36 s of which 0.35 s is
# the process's first GPU use; later calls' hooks, 11.8 GB fills included, take 0.01 s -- against 0.93 s for
# test_gpu_table_exact.py::test_key_table_tier[Ed25519-24] started the same way.  The time is the Python model
# (~4.5 ms a token for both chain orders and the big-integer reference), not the fill, so the random tokens were
# cut from 56 to 16 a call and every named edge token stays.  Inside the whole suite the cases then take
# 0.53 - 0.62 / 0.36 / 0.49 / 0.50 / 0.63 s at W = 24 / 22 / 20 / 18 / 16 against 0.39 - 0.40 s for the table case; the named
# tokens alone cost 0.29 - 0.56 s, so cutting the last 16 would not bring every case under it either.
NRAND = 8

_entries = {}                                      # (point, W) -> {(w, ad): words}, shared by the calls and forms
_model = {}                                        # (W, point, S, k) -> (one-lane X, Y, Z; split X, Y, Z)


@pytest.fixture(scope="module")
def tk():
    lib = ctypes.CDLL(os.path.join(ROOT, "cap_amd", "libcapjwt_tk.so"))
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.tk_ed_point.argtypes = [ctypes.c_int, i64, i64, i64, vp, vp, vp, vp, vp, ctypes.c_int, vp, vp, vp, i64, vp, vp,
                                vp, i64, vp, vp]
    assert lib.tk_ed_point_split_lanes() == ED_SPLIT, "the library was built with another JG_ED_SPLIT_LANES"
    return lib


class Slot:
    def __init__(self, tag, S, k, key=0, siglen=64, status=ST_OK, pad=False, rng=None):
        self.tag, self.S, self.k, self.key, self.siglen, self.status, self.pad = tag, S, k, key, siglen, status, pad
        # H = k + m L below 2^512: the kernel's k = H mod L is the k this token wants
        self.H = k + (rng.randrange((2**512 - k) // L) if rng else 0) * L
        assert self.H < 2**512 and self.H % L == k

    def s_ok(self):
        return M.ed_s_ok(self.S.to_bytes(32, "little"))

    def accepted(self, key_valid):
        return not self.pad and self.status == ST_OK and self.siglen == 64 and self.s_ok() and bool(key_valid[self.key])


def rejects(rng, key):
    r = lambda: rng.randrange(1, L)
    return [Slot("rej-S=L", L, r(), key, rng=rng), Slot("rej-S=L+1", L + 1, r(), key, rng=rng),
            Slot("rej-bit253", 5 | 2**253, r(), key, rng=rng), Slot("rej-bit254", (L - 1) | 2**254, r(), key, rng=rng),
            Slot("rej-bit255", r() | 2**255, r(), key, rng=rng), Slot("rej-siglen63", r(), r(), key, siglen=63, rng=rng),
            Slot("rej-siglen65", r(), r(), key, siglen=65, rng=rng),
            Slot("rej-status", r(), r(), key, status=ST_REJECT, rng=rng)]


def outside(rng):
    """a slot outside [begin, end): a live-looking ST_OK token, so a kernel that reached it would write"""
    return Slot("outside", rng.randrange(L), rng.randrange(L), 0, rng=rng)


def lay_out(groups, rng):
    """groups: two lists of live Slots (at most 64 less the fixed padding lanes
    each); returns the npad slots: every lane of a group without a token is a padding lane"""
    slots = [outside(rng) for _ in range(NPAD)]
    for g, live in enumerate(groups):
        key = live[0].key
        assert all(t.key == key for t in live)
        lanes = sorted(set(range(WAVE)) - pads_of(g))
        assert len(live) <= len(lanes), "more live tokens than lanes"
        # both neighbours of a padding lane inside a split wave take a token; the rest spread over the group
        first = [l for o in sorted(pads_of(g)) if 0 < o < WAVE - 1 for l in (o - 1, o + 1)]
        rest = [l for l in lanes if l not in first]
        at = dict(zip(first + rng.sample(rest, len(live) - len(first)), live))
        for lane in range(WAVE):
            slots[BEGIN + 64 * g + lane] = at.get(lane) or Slot("pad", 0, 0, key, pad=True)
    tokens_per_wave = WAVE // ED_SPLIT
    for o in PADS:                                                # a padding lane between live tokens of one split wave
        if 0 < o % WAVE < WAVE - 1:
            p = BEGIN + o
            assert slots[p].pad and not slots[p - 1].pad and not slots[p + 1].pad
            assert (p - 1) // tokens_per_wave == (p + 1) // tokens_per_wave
    return slots


def pads_of(g):
    return {o - 64 * g for o in PADS if 64 * g <= o < 64 * (g + 1)}


def main_slots(w, rng):
    two = w <= 20
    edge = E.tokens(w, 0, SECRET, seed=7)
    g1 = [Slot(tag, S, k, 0, rng=rng) for tag, S, k in edge]
    rj1, rj2 = rejects(rng, 0), rejects(rng, 1 if two else 0)
    g1 += rj1[:2] + rj1[4:6] + [rj1[7]]
    g2 = rj2[2:4] + rj2[5:]
    g2 += [Slot(tag + "-g2", S, k, g2[0].key, rng=rng) for tag, S, k in edge if tag.startswith(("k-pattern", "S=", "k="))]
    for g, live in enumerate((g1, g2)):
        assert len(live) + NRAND <= WAVE - len(pads_of(g))
        live += [Slot("random", rng.randrange(1, L), rng.randrange(1, L), live[0].key, rng=rng) for _ in range(NRAND)]
    return lay_out([g1, g2], rng)


def words_of(point, W, need):
    have = _entries.setdefault((point, W), {})
    have.update(E.entry_words(point, W, [wd for wd in need if wd not in have]))
    return have


def run_call(tk, w, slots, points, key_valid, label):
    """one hook call; asserts everything the module docstring lists; returns the times"""
    t0 = time.time()
    Bp = T.ed_base()
    acc = [p for p in range(BEGIN, END) if slots[p].accepted(key_valid)]
    dg = {p: E.digits(slots[p].S, slots[p].k, w) for p in acc}
    need_b = {(x, ad) for p in acc for s, x, ad in E.named_entries(*dg[p]) if s == 0}
    need_a = [{(x, ad) for p in acc if slots[p].key == k for s, x, ad in E.named_entries(*dg[p]) if s == 1}
              for k in range(len(points))]
    tab_b = words_of(Bp, M.ED_WB, need_b)
    tab_a = [words_of(points[k], w, need_a[k]) for k in range(len(points))]
    want = {}
    for p in acc:
        t = slots[p]
        key = (w, points[t.key], t.S, t.k)
        if key not in _model:
            entry = lambda side, x, ad: tab_a[t.key][(x, ad)] if side else tab_b[(x, ad)]
            _model[key] = (E.chain_one_lane(*dg[p], entry)[:3], E.chain_split(*dg[p], entry, ED_SPLIT)[:3])
        want[p] = _model[key]
    t_model = time.time() - t0

    t0 = time.time()
    jobs = np.zeros((NPAD, 4), dtype=np.uint32)
    st_in = np.zeros(NPAD, dtype=np.uint8)
    siglen = np.zeros(NPAD, dtype=np.uint16)
    srows = np.zeros((8, NPAD), dtype=np.uint32)
    dig = np.zeros((16, NPAD), dtype=np.uint32)
    for p, t in enumerate(slots):
        if t.pad:
            jobs[p, 3] = t.key | (JOB_PAD << 16)
            st_in[p], siglen[p] = 0xA5, 0xA5A5
            srows[:, p], dig[:, p] = POISON, POISON
            continue
        jobs[p, 3] = t.key | (ALG_EDDSA << 16) | (86 << 20)
        st_in[p], siglen[p] = t.status, t.siglen
        srows[:, p] = [(t.S >> (32 * q)) & 0xFFFFFFFF for q in range(8)]
        hb = t.H.to_bytes(64, "little")                       # the digest bytes; rows are big-endian words
        dig[:, p] = [int.from_bytes(hb[4 * q:4 * q + 4], "big") for q in range(16)]
    neb, nea = 1 << (M.ED_WB - 1), 1 << (w - 1)
    bl = sorted(need_b)
    b_idx = np.array([x * neb + ad - 1 for x, ad in bl], dtype=np.int64)
    b_ent = np.array([tab_b[wd] for wd in bl], dtype=np.uint32).reshape(len(bl), 32)
    al = [(k, x, ad) for k in range(len(points)) for x, ad in sorted(need_a[k])]
    a_key = np.array([k for k, _, _ in al], dtype=np.int64)
    a_idx = np.array([x * nea + ad - 1 for _, x, ad in al], dtype=np.int64)
    a_ent = np.array([tab_a[k][(x, ad)] for k, x, ad in al], dtype=np.uint32).reshape(len(al), 32)
    kv = np.array(key_valid, dtype=np.uint8)
    xyz = np.zeros((3, 30, NPAD), dtype=np.uint32)
    st_out = np.zeros((3, NPAD), dtype=np.uint8)
    rc = tk.tk_ed_point(w, NPAD, BEGIN, END, jobs.ctypes.data, st_in.ctypes.data, siglen.ctypes.data, srows.ctypes.data,
                        dig.ctypes.data, len(points), kv.ctypes.data, b_idx.ctypes.data, b_ent.ctypes.data, len(bl),
                        a_key.ctypes.data, a_idx.ctypes.data, a_ent.ctypes.data, len(al), xyz.ctypes.data,
                        st_out.ctypes.data)
    _die_on_hip_error(rc, "tk_ed_point")
    t_hook = time.time() - t0

    t0 = time.time()
    bad, seen = [], {"ok": 0, "rej": 0, "pad": 0}
    refs = {}
    for p, t in enumerate(slots):
        inside = BEGIN <= p < END
        for f in range(3):
            got = [[int(v) for v in xyz[f, 10 * c:10 * c + 10, p]] for c in range(3)]
            st = int(st_out[f, p])
            if not inside or t.pad:
                if any(v != POISON for c in got for v in c) or st != int(st_in[p]):
                    bad.append((p, t.tag, f, "padding / outside the launch, touched"))
                seen["pad"] += inside and f == 0
            elif p not in want:
                if st != ST_REJECT:
                    bad.append((p, t.tag, f, "status", st, "want ST_REJECT"))
                seen["rej"] += f == 0
            else:
                seen["ok"] += f == 0
                model = want[p][1 if f == 2 else 0]
                if got != model:
                    bad.append((p, t.tag, f, "limbs differ from the model", got, model))
                if st != ST_OK:
                    bad.append((p, t.tag, f, "status", st, "want ST_OK"))
                if not all(E.normalized(c) for c in got):
                    bad.append((p, t.tag, f, "a limb outside the normalized bound", got))
                if f != 1:                                    # (form 1's limbs are form 0's, asserted above)
                    if p not in refs:
                        refs[p] = E.reference(t.S, t.k, points[t.key])
                    if not E.same_point(got, refs[p]):
                        bad.append((p, t.tag, f, "not [S]B + [k](-A)"))
                if t.S == 0 and t.k == 0 and f != 2 and got != NEUTRAL_XYZ:
                    bad.append((p, t.tag, f, "S = k = 0 is not exactly (0, 1, 1)", got))
    t_cmp = time.time() - t0
    print(f"[ed-point-exact] W = {w} {label}: {seen['ok']} exact, {seen['rej']} rejected, {seen['pad']} padding; "
          f"{len(bl)} + {len(al)} entries; model {t_model:.2f} s, hook {t_hook:.2f} s, compare {t_cmp:.2f} s")
    # (the summary first: which tokens and forms failed; then the first few in full)
    assert not bad, (label, len(bad), sorted({(b[1], b[2], b[3]) for b in bad})[:40], bad[:3])
    return seen


def key0():
    return neg(T.ed_mul(SECRET, T.ed_base()))


def key1():
    """-A of a key of order 8, as the key staging decodes its 32 bytes"""
    q8 = order8_point()
    pt = T.ed_key_point((q8[1] | ((q8[0] & 1) << 255)).to_bytes(32, "little"))
    assert pt == neg(q8) and T.ed_mul(8, pt) == T.ED_IDENTITY != T.ed_mul(4, pt)
    return pt


@pytest.mark.parametrize("w", M.ED_WA)
def test_ed_point_exact(tk, w):
    rng = random.Random(0xED25519 + w)
    two = w <= 20
    points = [key0(), key1()] if two else [key0()]
    slots = main_slots(w, rng)
    tags = {t.tag for t in slots[BEGIN:END]}
    assert {"S=k=0", "sum-neutral-0", "sides-equal-0", "lane-S0-k1", "k-pattern-3", "S-pattern-3", "one-digit-k",
            "rej-S=L", "rej-S=L+1", "rej-bit253", "rej-bit254", "rej-bit255", "rej-siglen63", "rej-siglen65",
            "rej-status", "pad", "random"} <= tags
    assert two == any(t.key == 1 for t in slots[BEGIN:END])
    seen = run_call(tk, w, slots, points, [1] * len(points), "main")
    live = [sum(1 for t in slots[BEGIN + 64 * g:BEGIN + 64 * g + 64] if not t.pad) for g in range(2)]
    edge = E.tokens(w, 0, SECRET, seed=7)
    assert live == [len(edge) + 5 + NRAND, sum(t[0].startswith(("k-pattern", "S=", "k=")) for t in edge) + 5 + NRAND]
    assert seen == {"ok": sum(live) - 10, "rej": 10, "pad": 128 - sum(live)}
    # the special cases are what they claim (on the reference), and a single digit is one addition of its entry
    by = {t.tag: t for t in slots[BEGIN:END]}
    X, Y, Z, _ = E.reference(by["sum-neutral-0"].S, by["sum-neutral-0"].k, points[0])
    assert X % P == 0 and (Y - Z) % P == 0 and Z % P != 0
    assert T.ed_mul(by["sides-equal-0"].S, T.ed_base()) == T.ed_mul(by["sides-equal-0"].k, points[0])
    t = by["one-digit-S"]
    one = E.add_niels(E.neutral(), _entries[(T.ed_base(), M.ED_WB)][(1, 1)], 1)[:3]
    assert E.digits(t.S, t.k, w)[0][:3] == [0, 1, 0] and _model[(w, points[0], t.S, t.k)][0] == one
    if two:
        # key 1 invalid: group 2 rejects as a whole (its table holds poison alone), group 1 stays exact
        seen = run_call(tk, w, slots, points, [1, 0], "key 1 invalid")
        assert seen == {"ok": live[0] - 5, "rej": 5 + live[1], "pad": 128 - sum(live)}
    if w in (24, 16):
        # A = B and A = -B with S = k: every window pair cancels to the neutral element / adds the same
        # point twice (W = 24: equal widths, so inside the one-lane chain window by window)
        Bp = T.ed_base()
        us = [rng.randrange(1, L) for _ in range(2)] + [1, 1 << 48, (1 << 23) << 48, L - 1, 0, ed_patterns(24)[4]]
        calls = [[("A=B", neg(Bp)), ("A=-B", Bp)]] if w == 16 else [[("A=B", neg(Bp))], [("A=-B", Bp)]]
        for names in calls:
            groups = []
            for g in range(2):
                name, key = names[g % len(names)][0], g % len(names)
                mine = us if len(names) == 2 else us[g::2]           # (one key: the list is shared out)
                groups.append([Slot("%s S=k" % name, u, u, key, rng=rng) for u in mine] +
                              [Slot("%s random" % name, rng.randrange(L), rng.randrange(L), key, rng=rng)
                               for _ in range(2)])
            run_call(tk, w, lay_out(groups, rng), [q for _, q in names], [1] * len(names),
                     " + ".join(n for n, _ in names))


def test_hook_refuses_bad_arguments(tk):
    """each refusal returns -1 before anything is allocated or launched and leaves the outputs as passed in"""
    jobs = np.zeros((NPAD, 4), dtype=np.uint32)
    jobs[:, 3] = (ALG_EDDSA << 16) | (86 << 20)
    z8 = np.zeros(NPAD, dtype=np.uint8)
    sl = np.full(NPAD, 64, dtype=np.uint16)
    srows = np.zeros((8, NPAD), dtype=np.uint32)
    dig = np.zeros((16, NPAD), dtype=np.uint32)
    kv = np.ones(2, dtype=np.uint8)
    ent = np.zeros((1, 32), dtype=np.uint32)
    zero = np.zeros(1, dtype=np.int64)
    xyz = np.full((3, 30, NPAD), 0x5A5A5A5A, dtype=np.uint32)
    st = np.full((3, NPAD), 0x5A, dtype=np.uint8)

    def call(wa=16, end=END, nkeys=1, jobs=jobs, b_idx=zero, a_idx=zero, a_key=zero):
        return tk.tk_ed_point(wa, NPAD, BEGIN, end, jobs.ctypes.data, z8.ctypes.data, sl.ctypes.data, srows.ctypes.data,
                              dig.ctypes.data, nkeys, kv.ctypes.data, b_idx.ctypes.data, ent.ctypes.data, 1,
                              a_key.ctypes.data, a_idx.ctypes.data, ent.ctypes.data, 1, xyz.ctypes.data, st.ctypes.data)

    mixed = jobs.copy()
    mixed[BEGIN + 70, 3] |= 1                                  # one token of group 2 on key 1, the rest on key 0
    past = jobs.copy()
    past[BEGIN + 5, 3] |= 1                                    # key 1 with nkeys = 1
    at = lambda v: np.array([v], dtype=np.int64)
    for kw in (dict(wa=23), dict(wa=0), dict(end=200), dict(end=BEGIN), dict(end=NPAD + 64), dict(nkeys=3),
               dict(nkeys=0), dict(b_idx=at(11 << 23)), dict(b_idx=at(-1)), dict(a_idx=at(16 << 15)),
               dict(wa=24, a_idx=at(11 << 23)), dict(a_key=at(1)), dict(jobs=mixed, nkeys=2), dict(jobs=past)):
        assert call(**kw) == -1, kw
    assert (xyz == 0x5A5A5A5A).all() and (st == 0x5A).all()
