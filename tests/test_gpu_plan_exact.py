"""The dispatch-plan kernels of kernels/batch.hip alone, through the production
launchers (libcapjwt_tk.so: tk_plan_fill, tk_zc_gather, tk_copy, tk_scatter),
slot for slot against the plain model tests/plan_model.py -- which
tests/test_plan_model.py shows to refuse every single mistake.  Exact integer
work: no tolerance.  The pipeline behind these kernels only tells accept from
reject, and mostly on fresh buffers.

* Fill: the six invariants of plan_model.check_fill, on each of the three
  placement paths of launch_plan_fill (the one-level kernel, the two-level
  kernel for n > 4096 jobs over at most 2048 buckets, the one-level kernel on a
  large chunk over more buckets), at the sizes around every switch, for job
  patterns from one atomic target to 64 buckets per wave, with the field edges
  (alg 11..255, keys without a class, signature lengths around the clamp,
  offsets above 2^32) in every case, and into buffers a different chunk filled.
* Scatter: after a fill, and alone.
* Gather: every (off & 15, end & 15), three strides, padding in between, a
  sub-range, the grid-stride loop.
* Copy: both kernels, sizes around 16 bytes and a block, strided.
The buffers the kernels write are sentinel-filled with guard space, so slots
never written and writes outside the plan show."""
import array
import ctypes
import os
import random
import struct

import pytest

from tests import plan_model as PM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = PM.GUARD
U32MAX = (1 << 32) - 1


@pytest.fixture(scope="module")
def tk():
    L = ctypes.CDLL(os.path.join(ROOT, "cap_amd", "libcapjwt_tk.so"))
    vp, i64, u64, i32, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32
    L.tk_plan_fill.argtypes = [vp, i64, u64, vp, i32, vp, vp, i64, vp, vp, vp, vp, i32]
    L.tk_zc_gather.argtypes = [vp, u64, vp, i64, i64, i64, vp, vp, vp, i32, u64, vp, vp]
    L.tk_copy.argtypes = [vp, u32, u32, u64, vp, u32]
    L.tk_scatter.argtypes = [vp, vp, i64, i64, vp]
    return L


def buf(data):
    return ctypes.create_string_buffer(bytes(data), len(data))


def words(b, code):
    a = array.array(code)
    assert a.itemsize == {"I": 4, "i": 4, "Q": 8, "q": 8}[code]
    a.frombytes(bytes(b))
    return a


def jobs_of(b):
    return list(zip(*[iter(words(b, "I"))] * 4))


def pack_jobs(jobs):
    return array.array("I", [w for jb in jobs for w in jb]).tobytes()


# ---- fill ----

def cls_table(nkeys, dead=()):
    """key k: an RSA (algs 0..5), an EC (alg 6) or an Ed25519 (alg 9) key by k % 3; dead keys have no class"""
    tab = bytearray(nkeys * 16)
    for k in range(nkeys):
        if k in dead:
            continue
        for a in ((0, 1, 2, 3, 4, 5), (6,), (9,))[k % 3]:
            tab[k * 16 + a] = (2, 4, 7)[k % 3]
    return bytes(tab)


def plan_order(tab, nkeys):
    """the runtime's bucket order: class by class, key by key, the rejects last; keys without a class in no class"""
    cls = [max(tab[k * 16:k * 16 + 16]) for k in range(nkeys)]
    return sorted((k for k in range(nkeys) if cls[k]), key=lambda k: (cls[k], k)) + [nkeys]


SIGLENS = [86, 0, 342, 4094, 4095, 4096, U32MAX, 683]
RELS = [0, 101, U32MAX, 1 << 20]
REJECT_ALGS = [11, 12, 13, 14, 15, 16, 31, 255, 16 + 6, 16 + 9, 7, 10]


def make_toks(keys, base, tab, rejects_every=0):
    """one job per entry of keys; the field edges cycle through every case; every
    rejects_every-th job gets an alg its key has no class for"""
    toks = []
    for j, k in enumerate(keys):
        good = ((0, 1, 2, 3, 4, 5), (6,), (9,))[k % 3]
        alg = good[j % len(good)]
        if rejects_every and j % rejects_every == rejects_every - 1:
            alg = REJECT_ALGS[(j // rejects_every) % len(REJECT_ALGS)]
            if tab[k * 16 + alg] if alg < 16 else 0:
                alg = 255
        toks.append(PM.Tok(base + 5 + 977 * j, 17 + j % 4000, RELS[j % 4], SIGLENS[j % 8], k, alg))
    return toks


def pattern(name, n, nkeys, seed):
    rnd = random.Random(seed)
    if name == "one":
        return [0] * n
    if name == "rr":
        return [j % nkeys for j in range(n)]
    if name == "own":
        assert n <= nkeys
        return [(j * 7 + 3) % nkeys for j in range(n)] if nkeys % 7 else list(range(n))
    if name == "alt2":
        return [j % 2 for j in range(n)]
    if name == "wave64":                          # 64 different buckets in every wave
        assert nkeys >= 64
        return [(j % 64 + 64 * (j // 64)) % (nkeys // 64 * 64) for j in range(n)]
    if name in ("skew", "rejects"):
        return [int(nkeys * rnd.random() ** 3) for _ in range(n)]
    raise ValueError(name)


FILL_CASES = [
    (0, 1, "one"), (0, 33, "rr"), (0, 5000, "rr"),
    (1, 1, "one"), (1, 2, "rejects"), (1, 5000, "own"),
    (63, 2, "alt2"), (64, 33, "rr"), (65, 1, "one"), (65, 257, "wave64"),
    (255, 257, "own"), (256, 1, "one"), (256, 257, "wave64"), (257, 2, "alt2"), (257, 257, "own"),
    (1023, 33, "skew"), (1023, 5000, "own"), (1025, 257, "rr"), (1025, 2047, "own"),
    (4096, 1, "one"), (4096, 2, "rejects"), (4096, 33, "skew"), (4096, 2047, "wave64"), (4096, 5000, "own"),
    (4097, 1, "one"), (4097, 2, "alt2"), (4097, 33, "skew"), (4097, 33, "rejects"), (4097, 257, "wave64"),
    (4097, 2047, "rr"), (4097, 2048, "rr"), (4097, 5000, "own"),
    (5000, 2047, "skew"), (5000, 2048, "skew"),
    (5121, 2, "one"), (5121, 33, "rr"), (5121, 257, "skew"),
    (20000, 1, "one"), (20000, 33, "skew"), (20000, 2047, "wave64"), (20000, 5000, "skew"), (20011, 257, "rr"),
]


def fill_case(n, nkeys, name, seed=1):
    # "one", "alt2" and "wave64" are pure: exactly 1, 2 and 64 atomic targets per wave.  The others get keys
    # without a class (every 11th of a larger table), and "rr" and "skew" a reject in every 9th job.
    pure = name in ("one", "alt2", "wave64")
    dead = set(range(5, nkeys, 11)) if nkeys >= 33 and not pure else set()
    tab = cls_table(nkeys, dead)
    base = (3 << 32) + 4096 if seed % 2 else 0
    keys = pattern(name, n, nkeys, seed)
    toks = make_toks(keys, base, tab, rejects_every={"rejects": 1, "rr": 9, "skew": 9}.get(name, 0))
    if name == "rejects":
        assert all(PM.bucket(t, tab, nkeys) == nkeys for t in toks)
    if name == "wave64":
        assert all(len({PM.bucket(t, tab, nkeys) for t in toks[w:w + 64]}) == len(toks[w:w + 64])
                   for w in range(0, n, 64))
    lay = PM.layout(plan_order(tab, nkeys), PM.totals(toks, tab, nkeys))
    return toks, base, tab, lay


def run_fill(tk, toks, base, tab, nkeys, lay, cap=None, before=None, want_rc=0):
    """-> (jobs, perm, vpad, cursor), the whole buffers of cap + GUARD slots"""
    cap = lay.npad if cap is None else cap
    slots = cap + G
    raw = b"".join(struct.pack("<QIIIHBB", t.off, t.sig_in_len, t.sig_rel_off, t.sig_b64_len, t.key_idx, t.alg, 0)
                   for t in toks)
    cur_in = array.array("Q", lay.start).tobytes()
    pad = array.array("q", [x for r in lay.pad for x in r]).tobytes()
    if before is None:
        jb, pb, vb = buf(bytes(16 * slots)), buf(bytes(4 * slots)), buf(bytes(slots))
    else:
        jb, pb, vb = buf(pack_jobs(before[0])), buf(array.array("i", before[1]).tobytes()), buf(bytes(before[2]))
        assert len(jb) == 16 * slots and len(pb) == 4 * slots and len(vb) == slots
    cb = buf(bytes(8 * (nkeys + 1)))
    rc = tk.tk_plan_fill(buf(raw) if toks else None, len(toks), base, buf(tab) if nkeys else None, nkeys, buf(cur_in),
                         buf(pad), cap, jb, pb, vb, cb, 0 if before is None else 1)
    assert rc == want_rc
    return jobs_of(jb.raw), list(words(pb.raw, "i")), list(vb.raw), list(words(cb.raw, "Q"))


@pytest.mark.parametrize("n,nkeys,name", FILL_CASES,
                         ids=[f"{PM.fill_path(n, k)}-n{n}-k{k}-{p}" for n, k, p in FILL_CASES])
def test_fill(tk, n, nkeys, name):
    toks, base, tab, lay = fill_case(n, nkeys, name, seed=n + nkeys)
    jobs, perm, vpad, cur = run_fill(tk, toks, base, tab, nkeys, lay)
    PM.check_fill(toks, base, tab, nkeys, lay, jobs, perm, vpad, cur)


def test_fill_paths_covered():
    paths = {PM.fill_path(n, k) for n, k, _ in FILL_CASES}
    assert paths == {"one-level", "two-level", "one-level-large"}
    assert (4096, 2047, "wave64") in FILL_CASES and PM.fill_path(4096, 2047) == "one-level"
    assert PM.fill_path(4097, 2047) == "two-level" and PM.fill_path(5000, 2048) == "one-level-large"


@pytest.mark.parametrize("scale", [1, 40], ids=["one-level", "two-level"])
def test_fill_bucket_totals_mod_64(tk, scale):
    # bucket totals of 0, 1, 63, 64 and 65 mod 64 in one plan, empty buckets between full ones
    nkeys = 9
    counts = [0, 1, 63, 64, 65, 0, 128 * scale, 129 + 64 * scale, 0]
    tab = cls_table(nkeys)
    keys = [k for k, c in enumerate(counts) for _ in range(c)]
    random.Random(scale).shuffle(keys)
    toks = make_toks(keys, 1 << 40, tab) + [PM.Tok((1 << 40) + 9, 1, 2, 3, 4, 31)]      # one reject
    tot = PM.totals(toks, tab, nkeys)
    assert tot == counts + [1] and PM.fill_path(len(toks), nkeys) == ("one-level" if scale == 1 else "two-level")
    lay = PM.layout(plan_order(tab, nkeys), tot)
    jobs, perm, vpad, cur = run_fill(tk, toks, 1 << 40, tab, nkeys, lay)
    PM.check_fill(toks, 1 << 40, tab, nkeys, lay, jobs, perm, vpad, cur)


def test_fill_into_used_buffers(tk):
    """a buffer reused across chunks: each fill starts from what the last one left
    (another mix, another size, the other kernel) and leaves nothing stale inside
    its plan and everything outside it as it was"""
    nkeys = 33
    mixes = [fill_case(4500, nkeys, "skew", seed=1), fill_case(3000, nkeys, "rr", seed=2),
             fill_case(4097, nkeys, "skew", seed=3), fill_case(0, nkeys, "rr", seed=4)]
    assert [PM.fill_path(len(m[0]), nkeys) for m in mixes] == ["two-level", "one-level", "two-level", "one-level"]
    cap = max(m[3].npad for m in mixes) + 128
    state = None
    for toks, base, tab, lay in mixes:
        jobs, perm, vpad, cur = run_fill(tk, toks, base, tab, nkeys, lay, cap=cap, before=state)
        PM.check_fill(toks, base, tab, nkeys, lay, jobs, perm, vpad, cur, before=state)
        # as the pipeline leaves them: every live slot judged
        state = (jobs, perm, [1 if perm[p] >= 0 and p < lay.npad else v for p, v in enumerate(vpad)])


# ---- scatter ----

def run_scatter(tk, perm, vpad, ntok, want_rc=0):
    out = buf(bytes(ntok + 2 * G))
    rc = tk.tk_scatter(buf(array.array("i", perm).tobytes()), buf(bytes(vpad)), len(perm), ntok, out)
    assert rc == want_rc
    return out.raw


@pytest.mark.parametrize("n,nkeys,name", [(3000, 33, "skew"), (6000, 257, "skew")], ids=["one-level", "two-level"])
def test_fill_then_scatter(tk, n, nkeys, name):
    toks, base, tab, lay = fill_case(n, nkeys, name, seed=7)
    jobs, perm, vpad, cur = run_fill(tk, toks, base, tab, nkeys, lay)
    PM.check_fill(toks, base, tab, nkeys, lay, jobs, perm, vpad, cur)
    perm = perm[:lay.npad]
    verdicts = [(t * 131 + 7) & 1 if t >= 0 else 1 for t in perm]
    got = run_scatter(tk, perm, verdicts, n)
    assert got[:G] == got[-G:] == bytes([PM.BYTE_SENT]) * G
    assert list(got[G:G + n]) == [(j * 131 + 7) & 1 for j in range(n)]


@pytest.mark.parametrize("npad", [64, 256, 257 * 64])
def test_scatter_alone(tk, npad):
    rnd = random.Random(npad)
    ntok = npad + 37                                  # more caller slots than perm can name
    perm = rnd.sample(range(ntok), npad)
    for p in range(npad):
        if npad > 256 and (250 <= p < 262 or npad - 70 <= p):      # a run of padding over a block boundary, and the tail
            perm[p] = -1
        elif p % 64 >= 60:
            perm[p] = -1
    vpad = [rnd.randrange(0, 3) for _ in range(npad)]
    got = run_scatter(tk, perm, vpad, ntok)
    PM.check_scatter(perm, vpad, ntok, got)
    named = {t for t in perm if t >= 0}
    assert len(named) < ntok and all(got[G + t] == PM.BYTE_SENT for t in range(ntok) if t not in named)


# ---- gather ----

def gather_plan(specs, nkeys, seed=0):
    """specs: per padded slot None (padding) or (key, off & 15, input length, gap,
    signature length); slots of a key are consecutive.  -> the source bytes, the
    padded jobs and the per-key tables, with plan_chunk's stride rule."""
    rnd = random.Random(seed)
    src, jobs, kstart, kmax = bytearray(), [], [None] * nkeys, [0] * nkeys
    last = 0
    for p, s in enumerate(specs):
        if s is None:
            jobs.append(PM.pad_job(last, nkeys))
            continue
        key, a, n, gap, siglen = s
        last = key
        if kstart[key] is None:
            kstart[key] = p
        src += bytes((len(src) + 1) % 16 or 16 for _ in range(rnd.randrange(0, 5)))
        while len(src) % 16 != a:
            src.append(0x7E)
        off = len(src)
        src += rnd.randbytes(n) + bytes([0x2E]) * gap
        jobs.append((off, n, len(src), PM.pack(key, 6, siglen)))
        src += rnd.randbytes(min(siglen, PM.SIGLEN_MAX))
        kmax[key] = max(kmax[key], len(src) - off)
    kstart = [0 if s is None else s for s in kstart]
    kstride = [PM.zc_stride(m) if m else 0 for m in kmax]
    kbase, pos = [], 0
    for k in range(nkeys):
        kbase.append(pos)
        nslots = max((p + 1 for p, s in enumerate(specs) if s and s[0] == k), default=kstart[k]) - kstart[k]
        pos += (nslots + 63) // 64 * 64 * kstride[k]
    return bytes(src), jobs, kbase, kstart, kstride, pos


def run_gather(tk, src, jobs, begin, end, kbase, kstart, kstride, dst_len, want_rc=0):
    nk = len(kbase)
    jout, dout = buf(bytes(16 * (len(jobs) + G))), buf(bytes(dst_len + 2 * G))
    rc = tk.tk_zc_gather(buf(src), len(src), buf(pack_jobs(jobs)), len(jobs), begin, end,
                         buf(array.array("Q", kbase).tobytes()), buf(array.array("q", kstart).tobytes()),
                         buf(array.array("Q", kstride).tobytes()), nk, dst_len, jout, dout)
    assert rc == want_rc
    return jobs_of(jout.raw), dout.raw


def edge_specs():
    """every off & 15 x every end & 15, lengths 1 / 15 / 16 / 17 / ~700 by key,
    the signature right behind the input or after a gap, padding in between"""
    per_key = {0: [], 1: [], 2: []}
    i = 0
    for a in range(16):
        for e in range(16):
            key = i % 3
            n = ((1, 15, 16, 17), (697, 700, 703, 16), (17, 1, 15, 64))[key][(i // 3) % 4]
            gap = (0, 3, 0, 16)[(i // 5) % 4]
            siglen = 20 + (e - (a + n + gap + 20)) % 16                # so that the job ends at e mod 16
            assert (a + n + gap + siglen) % 16 == e
            per_key[key].append((key, a, n, gap, siglen))
            i += 1
    per_key[2].insert(40, (2, 9, 33, 1, 4095))                          # at the clamp
    per_key[2].insert(41, (2, 0, 16, 0, 4095 - 15))                     # one short of it, a whole number of 16-byte rows
    specs = []
    for key in range(3):
        for q, s in enumerate(per_key[key]):
            specs.append(s)
            if q % 13 == 5:
                specs.append(None)                                      # padding between live jobs
        while len(specs) % 64:
            specs.append(None)
    return specs


@pytest.mark.parametrize("sub", [False, True], ids=["whole", "sub-range"])
def test_gather_layout_edges(tk, sub):
    specs = edge_specs()
    src, jobs, kbase, kstart, kstride, dst_len = gather_plan(specs, 3)
    assert len(set(kstride)) == 3 and max(PM.job_siglen(jb) for jb in jobs) == 4095
    seen = {(jb[0] & 15, max(jb[0] + jb[1], jb[2] + PM.job_siglen(jb)) & 15) for jb in jobs if PM.job_live(jb)}
    assert len(seen) == 256
    begin, end = (70, len(jobs) - 70) if sub else (0, len(jobs))
    jout, dst = run_gather(tk, src, jobs, begin, end, kbase, kstart, kstride, dst_len)
    PM.check_gather(src, jobs, begin, end, kbase, kstart, kstride, dst_len, jout, dst)


def test_gather_last_job_ends_the_source(tk):
    # the aligned span of the last job reads up to 15 bytes into the slack behind the source
    specs = [(0, 5, 20, 0, 24)] * 3 + [None] * 61
    src, jobs, kbase, kstart, kstride, dst_len = gather_plan(specs, 1, seed=2)
    assert jobs[2][2] + PM.job_siglen(jobs[2]) == len(src) and len(src) % 16 == 1
    jout, dst = run_gather(tk, src, jobs, 0, 64, kbase, kstart, kstride, dst_len)
    PM.check_gather(src, jobs, 0, 64, kbase, kstart, kstride, dst_len, jout, dst)


def test_gather_grid_stride(tk):
    # more than 512 blocks * 256 lanes / 16 lanes per job = 8192 jobs: the grid-stride loop runs
    specs = []
    for key, cnt in enumerate((3000, 2900, 3100)):
        specs += [(key, (q * 5 + key) % 16, 10 + q % 23 + 9 * key, q % 2, 8 + q % 11) for q in range(cnt)]
        while len(specs) % 64:
            specs.append(None)
    assert sum(s is not None for s in specs) == 9000
    src, jobs, kbase, kstart, kstride, dst_len = gather_plan(specs, 3, seed=1)
    jout, dst = run_gather(tk, src, jobs, 0, len(jobs), kbase, kstart, kstride, dst_len)
    PM.check_gather(src, jobs, 0, len(jobs), kbase, kstart, kstride, dst_len, jout, dst)


# ---- copy ----

MIB = 1 << 20
COPY_SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097]
COPY_CASES = ([(s, d, b) for (s, d) in ((0, 0), (16, 32)) for b in COPY_SIZES + [16 * MIB + 23]] +
              [(s, d, b) for (s, d) in ((1, 0), (0, 8), (3, 3)) for b in COPY_SIZES + [MIB + 5]])


@pytest.fixture(scope="module")
def copy_source():
    return random.Random(9).randbytes(16 * MIB + 23)


@pytest.mark.parametrize("smis,dmis,nbytes", COPY_CASES,
                         ids=[f"{'copy16' if (s | d) % 16 == 0 else 'copy1'}-s{s}-d{d}-{b}" for s, d, b in COPY_CASES])
def test_copy(tk, copy_source, smis, dmis, nbytes):
    src = copy_source[:nbytes]
    out = buf(bytes(nbytes + 2 * G))
    assert tk.tk_copy(buf(src) if nbytes else None, smis, dmis, nbytes, out, G) == 0
    got = out.raw
    assert got[:G] == bytes([PM.BYTE_SENT]) * G and got[G + nbytes:] == bytes([PM.BYTE_SENT]) * G
    assert got[G:G + nbytes] == src


# ---- host and device decide the bucket by one rule ----

@pytest.mark.parametrize("copies", [1, 12], ids=["one-level", "two-level"])
def test_host_and_device_agree_on_algs_past_the_table(copies):
    """plan_count / scan_chunk count the buckets on the host, the fill kernels
    place into them on the device: a job whose alg is 11..15, 16, its own alg +
    16 (the same low four bits), 31 or 255 must be a reject for both, or the
    device runs a bucket over into its neighbour.  Valid tokens, each beside
    copies of itself with such an alg: only the originals verify, through the
    pipeline (device fill) and as a resident batch (host fill)."""
    from cap_amd import _lib
    from tests import gpu_helpers as H
    keys, toks = H.golden()
    kid_index = {k["kid"]: i for i, k in enumerate(keys)}
    sel = [t for t in toks if t["name"].startswith("valid-")][::2]      # every key class
    arena, slots = H.jobs_from_tokens(sel, kid_index)
    assert None not in slots and len(slots) == 40
    jobs, want = [], []
    for r in range(copies):
        for s in slots:
            off, n, rel, siglen, key, alg = arena.toks[s]
            assert alg <= 10
            for a in (alg, 11, 12, 13, 14, 15, 16, alg + 16, 31, 255, alg | 0xF0):
                jobs.append((off, n, rel, siglen, key, a))
                want.append(1 if a == alg else 0)
    order = list(range(len(jobs)))
    random.Random(copies).shuffle(order)
    mixed = _lib.Arena()
    mixed.buf = arena.buf
    mixed.toks = [jobs[i] for i in order]
    want = bytes(want[i] for i in order)
    assert PM.fill_path(len(jobs), len(keys)) == ("one-level" if copies == 1 else "two-level")
    ctx = _lib.Context()
    try:
        ctx.load_keys([H.abi_key(k) for k in keys])
        assert ctx.verify(mixed) == want
        b = ctx.stage(mixed)
        try:
            assert b.run(True) == want
        finally:
            b.free()
    finally:
        ctx.close()


# ---- the hooks' own argument checks ----

def test_hooks_refuse_plans_outside_their_buffers(tk):
    nkeys = 3
    tab = cls_table(nkeys)
    toks = make_toks([0, 1, 2, 1], 0, tab)
    lay = PM.layout(plan_order(tab, nkeys), PM.totals(toks, tab, nkeys))
    zero = ([(0, 0, 0, 0)] * (lay.npad + G), [0] * (lay.npad + G), [0] * (lay.npad + G), [0] * (nkeys + 1))
    ok = run_fill(tk, toks, 0, tab, nkeys, lay)
    PM.check_fill(toks, 0, tab, nkeys, lay, *ok)
    # key_idx >= nkeys
    bad = toks[:2] + [toks[2]._replace(key_idx=nkeys)] + toks[3:]
    assert run_fill(tk, bad, 0, tab, nkeys, lay, want_rc=-1) == zero
    # a bucket's jobs past npad; its padding past npad
    far = lay._replace(start=[lay.start[0], lay.npad - 1, lay.start[2], lay.start[3]])
    assert run_fill(tk, toks, 0, tab, nkeys, far, want_rc=-1) == zero
    far = lay._replace(pad=lay.pad[:2] + [(lay.pad[2][0], lay.npad + 1)] + lay.pad[3:])
    assert run_fill(tk, toks, 0, tab, nkeys, far, want_rc=-1) == zero
    assert run_fill(tk, toks, 0, tab, nkeys, lay, cap=lay.npad - 64, want_rc=-1)[0] == zero[0][:-64]

    specs = [(0, 3, 40, 0, 30)] * 5 + [None] * 59
    src, jobs, kbase, kstart, kstride, dst_len = gather_plan(specs, 1)
    jout, dst = run_gather(tk, src, jobs, 0, 64, kbase, kstart, kstride, dst_len)
    PM.check_gather(src, jobs, 0, 64, kbase, kstart, kstride, dst_len, jout, dst)
    untouched = ([(0, 0, 0, 0)] * (64 + G), bytes(4 * kstride[0] + 2 * G))
    # the fifth job's slot past dst_len; a span past the source; a key past the table; a stride not of 16
    assert run_gather(tk, src, jobs, 0, 64, kbase, kstart, kstride, 4 * kstride[0], want_rc=-1) == untouched
    untouched = ([(0, 0, 0, 0)] * (64 + G), bytes(dst_len + 2 * G))
    assert run_gather(tk, src[:-1], jobs, 0, 64, kbase, kstart, kstride, dst_len, want_rc=-1) == untouched
    other = [jobs[0][:3] + (jobs[0][3] | 1,)] + jobs[1:]
    assert run_gather(tk, src, other, 0, 64, kbase, kstart, kstride, dst_len, want_rc=-1) == untouched
    assert run_gather(tk, src, jobs, 0, 64, kbase, kstart, [kstride[0] + 8], dst_len, want_rc=-1) == untouched
    assert run_gather(tk, src, jobs, 0, 65, kbase, kstart, kstride, dst_len, want_rc=-1) == untouched

    assert run_scatter(tk, [0, 1, 4, -1], [1, 1, 1, 1], 4, want_rc=-1) == bytes(4 + 2 * G)
    assert run_scatter(tk, [0, 1, 3, -1], [1, 1, 1, 1], 4)[G:G + 4] == bytes([1, 1, PM.BYTE_SENT, 1])
    out = buf(bytes(16 + 2 * G))
    assert tk.tk_copy(buf(bytes(16)), 256, 0, 16, out, G) == -1 and out.raw == bytes(16 + 2 * G)
