"""tests/plan_model.py on the CPU: its checkers accept the result of a plain
sequential fill and gather written here, and refuse every single mistake a
placement or gather kernel could make -- so tests/test_gpu_plan_exact.py would
fail on a subtly wrong kernel, and no kernel has to be broken to show it."""
import random

import pytest

from tests import plan_model as PM

NKEYS = 5
BASE = (1 << 32) + 256


def cls_table():
    tab = bytearray(NKEYS * 16)
    for a in range(0, 6):
        tab[0 * 16 + a] = 1                      # key 0: an RSA key
    for a in range(0, 6):
        tab[1 * 16 + a] = 3
    tab[2 * 16 + 6] = 4                          # key 2: P-256; key 3: invalid, all zero
    tab[4 * 16 + 9] = 7                          # key 4: Ed25519
    return bytes(tab)


def chunk():
    rnd = random.Random(11)
    toks = []
    for j in range(300):
        key = rnd.choice([0, 0, 0, 1, 2, 2, 3, 4])
        alg = rnd.choice({0: [0, 3, 5, 6], 1: [1, 2], 2: [6, 6, 6, 7], 3: [0, 6], 4: [9, 9, 10]}[key])
        toks.append(PM.Tok(BASE + 40 + 700 * j, 100 + j, 101 + j, rnd.choice([0, 86, 342, 4094, 4095]), key, alg))
    # the field edges: alg past the table, a long signature, a wrapped offset
    toks[5] = toks[5]._replace(key_idx=4, alg=31, sig_b64_len=342)
    toks[6] = toks[6]._replace(key_idx=2, alg=16)
    toks[7] = toks[7]._replace(key_idx=1, alg=255)
    toks[8] = toks[8]._replace(key_idx=0, alg=0, sig_b64_len=4096)
    toks[9] = toks[9]._replace(key_idx=0, alg=0, sig_b64_len=(1 << 32) - 1)
    toks[10] = toks[10]._replace(key_idx=2, alg=6, off=BASE + 3, sig_rel_off=(1 << 32) - 2)
    return toks


def fill_ref(toks, base, tab, nkeys, lay):
    """the plan, placed one job after another"""
    slots = lay.npad + PM.GUARD
    jobs, perm, vpad = [PM.JOB_SENT] * slots, [PM.PERM_SENT] * slots, [PM.BYTE_SENT] * slots
    cur = list(lay.start)
    for j, t in enumerate(toks):
        b = PM.bucket(t, tab, nkeys)
        p = cur[b]
        cur[b] += 1
        o = (t.off - base) % (1 << 64)
        meta = (0 if b == nkeys else t.key_idx) | (t.alg % 16) << 16 | min(t.sig_b64_len, 4095) << 20
        jobs[p], perm[p], vpad[p] = (o % (1 << 32), t.sig_in_len, (o + t.sig_rel_off) % (1 << 32), meta), j, 0
    for b, (lo, hi) in enumerate(lay.pad):
        for p in range(lo, hi):
            jobs[p], perm[p], vpad[p] = (0, 0, 0, (0 if b == nkeys else b) | 15 << 16), -1, 0
    return jobs, perm, vpad, cur


@pytest.fixture()
def filled():
    tab, toks = cls_table(), chunk()
    tot = PM.totals(toks, tab, NKEYS)
    assert all(tot[b] >= 2 for b in (0, 1, 2, 4, NKEYS)) and tot[3] == 0
    lay = PM.layout([0, 1, 2, 4, NKEYS], tot)
    jobs, perm, vpad, cur = fill_ref(toks, BASE, tab, NKEYS, lay)
    return dict(toks=toks, tab=tab, lay=lay, jobs=jobs, perm=perm, vpad=vpad, cur=cur)


def run_check(f, **kw):
    PM.check_fill(f["toks"], BASE, f["tab"], NKEYS, f["lay"], f["jobs"], f["perm"], f["vpad"], f["cur"], **kw)


def slot_of(f, j):
    return f["perm"].index(j)


def test_layout():
    lay = PM.layout([2, 0, 3], [65, 0, 64, 1])
    assert lay.start == [64, 0, 0, 192] and lay.npad == 256
    assert lay.pad == [(129, 192), (0, 0), (64, 64), (193, 256)]
    lay = PM.layout([1, 0, 2], [0, 63, 0])                   # empty buckets between full ones
    assert lay.start == [64, 0, 64] and lay.pad == [(64, 64), (63, 64), (64, 64)] and lay.npad == 64
    lay = PM.layout([0, 1, 2], [0, 0, 0])                    # the empty plan: one wave in the reject bucket
    assert lay.npad == 64 and lay.pad == [(0, 0), (0, 0), (0, 64)] and lay.start == [0, 0, 0]
    with pytest.raises(AssertionError):
        PM.layout([0, 2], [1, 1, 0])                         # a bucket with jobs left out of the order


def test_rules():
    tab = cls_table()
    T = PM.Tok
    assert PM.bucket(T(0, 0, 0, 0, 0, 5), tab, NKEYS) == 0
    assert PM.bucket(T(0, 0, 0, 0, 0, 6), tab, NKEYS) == NKEYS          # alg / key mismatch
    assert PM.bucket(T(0, 0, 0, 0, 3, 0), tab, NKEYS) == NKEYS          # a key with no class
    for alg in (11, 12, 13, 14, 15, 16, 31, 255):
        assert PM.bucket(T(0, 0, 0, 0, 4, alg), tab, NKEYS) == NKEYS
    assert PM.bucket(T(0, 0, 0, 0, 4, 9), tab, NKEYS) == 4
    # alg 16 + 9 must not be read as alg 9: the table is not indexed past a key's row
    assert PM.bucket(T(0, 0, 0, 0, 3, 16 + 9), tab, NKEYS) == NKEYS
    assert PM.expected_job(T(BASE + 7, 20, 21, 4096, 4, 9), BASE, tab, NKEYS) == (7, 20, 28, 4 | 9 << 16 | 4095 << 20)
    assert PM.expected_job(T(BASE + 7, 20, 21, 4094, 4, 31), BASE, tab, NKEYS) == (7, 20, 28, 15 << 16 | 4094 << 20)
    assert PM.expected_job(T(3, 1, 2, 0, 2, 6), 4, tab, NKEYS) == (0xFFFFFFFF, 1, 1, 2 | 6 << 16)
    assert PM.pad_job(3, NKEYS) == (0, 0, 0, 3 | 15 << 16) and PM.pad_job(NKEYS, NKEYS) == (0, 0, 0, 15 << 16)
    assert [PM.zc_stride(k) for k in (0, 1, 3, 4, 19, 20)] == [32, 32, 48, 48, 64, 64]
    assert PM.fill_path(4096, 1) == "one-level" and PM.fill_path(4097, 2047) == "two-level"
    assert PM.fill_path(4097, 2048) == "one-level-large" and PM.fill_path(0, 5000) == "one-level"


def test_fill_accepted(filled):
    run_check(filled)
    # free order inside a bucket: any permutation of a bucket's slots is the same plan
    s, n = filled["lay"].start[0], filled["lay"].total[0]
    order = list(range(s, s + n))
    random.Random(3).shuffle(order)
    for name in ("jobs", "perm", "vpad"):
        filled[name][s:s + n] = [filled[name][p] for p in order]
    run_check(filled)


def test_fill_accepted_on_a_reused_buffer(filled):
    # slots outside the new plan keep what the last chunk left there
    slots = filled["lay"].npad + PM.GUARD + 128
    old = ([(p, 2, 3, 4) for p in range(slots)], list(range(slots)), [p % 251 for p in range(slots)])
    for name, o in zip(("jobs", "perm", "vpad"), old):
        filled[name] = filled[name][:filled["lay"].npad] + o[filled["lay"].npad:]
    run_check(filled, before=old)
    with pytest.raises(AssertionError):
        run_check(filled)
    filled["vpad"][filled["lay"].npad + 70] ^= 1
    with pytest.raises(AssertionError):
        run_check(filled, before=old)


def test_empty_plan():
    tab = cls_table()
    lay = PM.layout([0, 1, 2, 4, NKEYS], [0] * (NKEYS + 1))
    jobs, perm, vpad, cur = fill_ref([], 0, tab, NKEYS, lay)
    PM.check_fill([], 0, tab, NKEYS, lay, jobs, perm, vpad, cur)
    assert jobs[:64] == [(0, 0, 0, 15 << 16)] * 64
    jobs[63] = PM.JOB_SENT
    with pytest.raises(AssertionError):
        PM.check_fill([], 0, tab, NKEYS, lay, jobs, perm, vpad, cur)


def m_dup_perm(f):
    s = f["lay"].start[1]
    f["perm"][s + 1], f["jobs"][s + 1] = f["perm"][s], f["jobs"][s]


def m_swap_across_buckets(f):
    # keys 0 and 1 share every alg of this swap's jobs, so only the key tells them apart
    a, b = f["lay"].start[0], f["lay"].start[1]
    for name in ("jobs", "perm"):
        f[name][a], f[name][b] = f[name][b], f[name][a]


def m_job_in_pad_range(f):
    lo, hi = f["lay"].pad[2]
    assert hi - lo >= 1
    for name in ("jobs", "perm", "vpad"):
        f[name][lo - 1], f[name][lo] = f[name][lo], f[name][lo - 1]


def m_stale_pad(f):
    lo, hi = f["lay"].pad[4]
    f["jobs"][hi - 1] = f["jobs"][f["lay"].start[4]]           # what an earlier chunk left: a live job of this key


def m_stale_pad_perm(f):
    f["perm"][f["lay"].pad[NKEYS][1] - 1] = 0


def m_vpad_filled(f):
    f["vpad"][f["lay"].start[2] + 1] = 1


def m_vpad_pad(f):
    f["vpad"][f["lay"].pad[0][0]] = 1


def m_off_not_rebased(f):
    p = slot_of(f, 20)
    t, jb = f["toks"][20], f["jobs"][p]
    f["jobs"][p] = (t.off & PM.M32, jb[1], (t.off + t.sig_rel_off) & PM.M32, jb[3])


def m_sig_off_without_rel(f):
    p = slot_of(f, 21)
    jb = f["jobs"][p]
    f["jobs"][p] = (jb[0], jb[1], jb[0], jb[3])


def m_key_kept_for_reject(f):
    p = slot_of(f, 7)                                          # key 1, alg 255
    assert f["lay"].start[NKEYS] <= p
    jb = f["jobs"][p]
    f["jobs"][p] = jb[:3] + (jb[3] | 1,)


def m_alg_not_masked(f):
    p = slot_of(f, 5)                                          # alg 31, an even signature length
    t, jb = f["toks"][5], f["jobs"][p]
    f["jobs"][p] = jb[:3] + (t.alg << 16 | t.sig_b64_len << 20,)


def m_siglen_not_clamped(f):
    p = slot_of(f, 8)                                          # 4096 characters
    t, jb = f["toks"][8], f["jobs"][p]
    f["jobs"][p] = jb[:3] + ((t.key_idx | t.alg << 16 | t.sig_b64_len << 20) & PM.M32,)


def m_cursor_plus(f):
    f["cur"][2] += 1


def m_cursor_minus(f):
    f["cur"][NKEYS] -= 1


def m_guard_job(f):
    f["jobs"][f["lay"].npad] = (0, 0, 0, 15 << 16)


def m_guard_perm(f):
    f["perm"][f["lay"].npad + PM.GUARD - 1] = -1


def m_guard_vpad(f):
    f["vpad"][f["lay"].npad + 1] = 0


FILL_MUTATIONS = [m_dup_perm, m_swap_across_buckets, m_job_in_pad_range, m_stale_pad, m_stale_pad_perm, m_vpad_filled,
                  m_vpad_pad, m_off_not_rebased, m_sig_off_without_rel, m_key_kept_for_reject, m_alg_not_masked,
                  m_siglen_not_clamped, m_cursor_plus, m_cursor_minus, m_guard_job, m_guard_perm,
                  m_guard_vpad]


@pytest.mark.parametrize("mutate", FILL_MUTATIONS, ids=lambda m: m.__name__[2:])
def test_fill_mutation_refused(filled, mutate):
    mutate(filled)
    with pytest.raises(AssertionError):
        run_check(filled)


# ---- the gather ----

def gather_case():
    rnd = random.Random(5)
    kstart = [0, 64, 128]
    jobs, src = [], bytearray()
    lens = {0: 40, 1: 300, 2: 17}
    for p in range(192):
        key = p // 64
        if p % 64 >= 50 or p % 7 == 3:                           # padding at the end of a bucket and in between
            jobs.append(PM.pad_job(key, 3))
            continue
        src += bytes(rnd.randrange(1, 0xA5) for _ in range(rnd.randrange(0, 23)))
        off, n = len(src), lens[key] + p % 5
        src += bytes(rnd.randrange(1, 0xA5) for _ in range(n))
        gap = (p % 3) * 2
        src += bytes(gap)
        siglen = 22 + p % 9
        jobs.append((off, n, len(src), PM.pack(key, 6, siglen)))
        src += bytes(rnd.randrange(1, 0xA5) for _ in range(siglen))
    kmax = [max(jb[2] + PM.job_siglen(jb) - jb[0] for jb in jobs[k * 64:k * 64 + 64] if PM.job_live(jb)) for k in range(3)]
    kstride = [PM.zc_stride(m) for m in kmax]
    kbase = [0, 64 * kstride[0], 64 * (kstride[0] + kstride[1])]
    return dict(src=bytes(src), jobs=jobs, begin=10, end=180, kbase=kbase, kstart=kstart, kstride=kstride,
                dst_len=64 * sum(kstride))


def gather_ref(g):
    """the gather, one job after another: the aligned span around each live job"""
    src = g["src"] + bytes(256)
    dst = bytearray([PM.BYTE_SENT]) * (g["dst_len"] + 2 * PM.GUARD)
    out = list(g["jobs"]) + [PM.JOB_SENT] * PM.GUARD
    for p in range(g["begin"], g["end"]):
        off, n, sig, meta = g["jobs"][p]
        if meta >> 16 & 15 == 15:
            continue
        key = meta & 0xFFFF
        lo, hi = off // 16 * 16, -(-max(off + n, sig + (meta >> 20)) // 16) * 16
        d0 = g["kbase"][key] + (p - g["kstart"][key]) * g["kstride"][key]
        dst[PM.GUARD + d0:PM.GUARD + d0 + hi - lo] = src[lo:hi]
        out[p] = (d0 + off - lo, n, d0 + sig - lo, meta)
    return out, dst


def run_gather_check(g, out, dst):
    PM.check_gather(g["src"], g["jobs"], g["begin"], g["end"], g["kbase"], g["kstart"], g["kstride"], g["dst_len"], out,
                    dst)


def live(g, k=0):
    return [p for p in range(g["begin"], g["end"]) if PM.job_live(g["jobs"][p])][k]


def test_gather_accepted():
    g = gather_case()
    out, dst = gather_ref(g)
    assert any(out[p] != g["jobs"][p] for p in range(192))
    run_gather_check(g, out, dst)
    # a gather that copies the jobs' own bytes and nothing around them is as good
    exact = bytearray([PM.BYTE_SENT]) * len(dst)
    for p in range(g["begin"], g["end"]):
        if PM.job_live(g["jobs"][p]):
            off, n, sig, meta = out[p]
            exact[PM.GUARD + off:PM.GUARD + sig + (meta >> 20)] = dst[PM.GUARD + off:PM.GUARD + sig + (meta >> 20)]
    run_gather_check(g, out, exact)


def g_shifted_by_16(g, out, dst):
    p = live(g, 4)
    d0, lo, hi = PM.gather_slot(g["jobs"][p], p, g["kbase"], g["kstart"], g["kstride"])
    span = dst[PM.GUARD + d0:PM.GUARD + d0 + hi - lo]
    dst[PM.GUARD + d0:PM.GUARD + d0 + 16] = bytes([PM.BYTE_SENT]) * 16
    dst[PM.GUARD + d0 + 16:PM.GUARD + d0 + 16 + hi - lo] = span
    out[p] = (out[p][0] + 16, out[p][1], out[p][2] + 16, out[p][3])


def g_bytes_shifted_offsets_not(g, out, dst):
    p = live(g, 4)
    d0, lo, hi = PM.gather_slot(g["jobs"][p], p, g["kbase"], g["kstart"], g["kstride"])
    dst[PM.GUARD + d0 + 16:PM.GUARD + d0 + 16 + hi - lo] = dst[PM.GUARD + d0:PM.GUARD + d0 + hi - lo]


def g_byte_past_span(g, out, dst):
    p = live(g, 9)
    d0, lo, hi = PM.gather_slot(g["jobs"][p], p, g["kbase"], g["kstart"], g["kstride"])
    assert dst[PM.GUARD + d0 + hi - lo] == PM.BYTE_SENT
    dst[PM.GUARD + d0 + hi - lo] = 0


def g_byte_before_span(g, out, dst):
    p = live(g, 9)
    d0, lo, hi = PM.gather_slot(g["jobs"][p], p, g["kbase"], g["kstart"], g["kstride"])
    dst[PM.GUARD + d0 - 1] = 0


def g_pad_rewritten(g, out, dst):
    p = next(p for p in range(g["begin"], g["end"]) if not PM.job_live(g["jobs"][p]))
    out[p] = (g["kbase"][1], 0, g["kbase"][1], out[p][3])


def g_job_outside_range(g, out, dst):
    p = g["begin"] - 1
    while not PM.job_live(g["jobs"][p]):
        p -= 1
    d0, lo, hi = PM.gather_slot(g["jobs"][p], p, g["kbase"], g["kstart"], g["kstride"])
    out[p] = (d0 + out[p][0] - lo, out[p][1], d0 + out[p][2] - lo, out[p][3])


def g_off_not_rewritten(g, out, dst):
    p = live(g, 2)
    out[p] = g["jobs"][p]


def g_wrong_byte(g, out, dst):
    p = live(g, 30)
    dst[PM.GUARD + out[p][2] + PM.job_siglen(out[p]) - 1] ^= 0x40    # the signature's last character


def g_low_guard(g, out, dst):
    dst[PM.GUARD - 1] = 0


def g_high_guard(g, out, dst):
    dst[-PM.GUARD] = 0


def g_guard_job(g, out, dst):
    out[len(g["jobs"])] = (0, 0, 0, 0)


GATHER_MUTATIONS = [g_shifted_by_16, g_bytes_shifted_offsets_not, g_byte_past_span, g_byte_before_span, g_pad_rewritten,
                    g_job_outside_range, g_off_not_rewritten, g_wrong_byte, g_low_guard, g_high_guard, g_guard_job]


@pytest.mark.parametrize("mutate", GATHER_MUTATIONS, ids=lambda m: m.__name__[2:])
def test_gather_mutation_refused(mutate):
    g = gather_case()
    out, dst = gather_ref(g)
    mutate(g, out, dst)
    with pytest.raises(AssertionError):
        run_gather_check(g, out, dst)


def test_scatter_checker():
    perm = [2, -1, 0, -1]
    PM.check_scatter(perm, [1, 1, 0, 1], 4, bytes([0xA5] * 64 + [0, 0xA5, 1, 0xA5] + [0xA5] * 64))
    with pytest.raises(AssertionError):
        PM.check_scatter(perm, [1, 1, 0, 1], 4, bytes([0xA5] * 64 + [0, 1, 1, 0xA5] + [0xA5] * 64))
    with pytest.raises(AssertionError):
        PM.check_scatter(perm, [1, 1, 0, 1], 4, bytes([0xA5] * 63 + [0] + [0, 0xA5, 1, 0xA5] + [0xA5] * 64))
