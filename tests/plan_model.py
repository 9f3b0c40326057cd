"""Plain model of a pipeline chunk's dispatch plan (no GPU, no project code):
what the kernels of cap_amd/csrc/kernels/batch.hip must leave in HBM, restated
from the rule, and the checkers the device tests (tests/test_gpu_plan_exact.py)
hold them to.  tests/test_plan_model.py shows on the CPU that the checkers
accept a correct result and refuse every single mistake a kernel could make.

The plan.  A chunk's jobs are sorted by bucket: bucket k < nkeys holds the jobs
of key k whose (key, alg) pair has a kernel class, bucket nkeys the rejects
(class 0: cls_tab[key * 16 + alg] == 0, or alg >= 16).  Every bucket is padded
to whole waves of 64 slots; the empty plan is one wave of padding in the reject
bucket.  Slot p holds a 16-byte job (off, sig_in_len, sig_off, meta), perm[p]
names the caller's job in that slot (-1: padding) and vpad[p] is the slot's
verdict byte, zeroed by the fill.  The order inside a bucket is free.

    off      = (tok.off - base) mod 2^32
    sig_off  = (tok.off - base + tok.sig_rel_off) mod 2^32
    meta     = key | (alg & 15) << 16 | min(sig_b64_len, 4095) << 20
               key is 0 for a reject; a padding slot is (0, 0, 0, pack(b or 0, 15, 0))

Jobs are 4-tuples of ints, toks are Tok tuples, buffers are plain sequences."""
from collections import namedtuple

WAVE = 64
GUARD = 64                          # guard slots behind slot arrays, guard bytes around byte buffers
JOB_PAD = 15
SIGLEN_MAX = 4095
NALG = 16
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
JOB_SENT = (0xA5A5A5A5,) * 4        # the hooks' sentinel: 0xA5 bytes, perm 0x5A5A5A5A
PERM_SENT = 0x5A5A5A5A
BYTE_SENT = 0xA5
PF_MAX_BUCKETS, PF_SMALL = 2048, 4096   # launch_plan_fill's rule

Tok = namedtuple("Tok", "off sig_in_len sig_rel_off sig_b64_len key_idx alg")
Layout = namedtuple("Layout", "start total pad npad")


def pack(key, alg, siglen):
    return (key & 0xFFFF) | (alg & 15) << 16 | min(siglen, SIGLEN_MAX) << 20


def job_key(job):
    return job[3] & 0xFFFF


def job_alg(job):
    return job[3] >> 16 & 15


def job_siglen(job):
    return job[3] >> 20


def job_live(job):
    return job_alg(job) != JOB_PAD


def pad_job(b, nkeys):
    return (0, 0, 0, pack(0 if b == nkeys else b, JOB_PAD, 0))


def bucket(tok, cls_tab, nkeys):
    assert tok.key_idx < nkeys
    c = cls_tab[tok.key_idx * NALG + tok.alg] if tok.alg < NALG else 0
    return nkeys if c == 0 else tok.key_idx


def expected_job(tok, base, cls_tab, nkeys):
    o = (tok.off - base) & M64
    key = 0 if bucket(tok, cls_tab, nkeys) == nkeys else tok.key_idx
    return (o & M32, tok.sig_in_len, (o + tok.sig_rel_off) & M32, pack(key, tok.alg, tok.sig_b64_len))


def totals(toks, cls_tab, nkeys):
    tot = [0] * (nkeys + 1)
    for t in toks:
        tot[bucket(t, cls_tab, nkeys)] += 1
    return tot


def layout(buckets, total):
    """buckets: the buckets in plan order (the runtime: class by class, key by
    key, the reject bucket -- the last one, len(total) - 1 -- at the end);
    total[b]: jobs per bucket.  A bucket the order leaves out must be empty and
    gets start 0 and no padding, as a key without a kernel class does."""
    nb = len(total)
    assert len(set(buckets)) == len(buckets) and all(0 <= b < nb for b in buckets)
    assert all(total[b] == 0 for b in range(nb) if b not in set(buckets))
    start, pad, pos = [0] * nb, [(0, 0)] * nb, 0
    for b in buckets:
        start[b] = pos
        pos += (total[b] + WAVE - 1) // WAVE * WAVE
        pad[b] = (start[b] + total[b], pos)
    if pos == 0:                                  # the empty plan: one wave of padding
        pad[nb - 1] = (0, WAVE)
        pos = WAVE
    return Layout(start, list(total), pad, pos)


def fill_path(n, nkeys):
    """the kernel launch_plan_fill picks"""
    if n > PF_SMALL and nkeys + 1 <= PF_MAX_BUCKETS:
        return "two-level"
    return "one-level-large" if n > PF_SMALL else "one-level"


def check_fill(toks, base, cls_tab, nkeys, lay, jobs, perm, vpad, cursor, before=None):
    """The six invariants of a plan fill.  jobs / perm / vpad: the whole
    buffers, guards included.  before: their contents ahead of the fill
    (default: the sentinel everywhere)."""
    slots = len(jobs)
    assert len(perm) == slots and len(vpad) == slots and slots >= lay.npad + GUARD
    assert lay.total == totals(toks, cls_tab, nkeys), "the layout is not this chunk's"
    want = [[] for _ in range(nkeys + 1)]
    for j, t in enumerate(toks):
        want[bucket(t, cls_tab, nkeys)].append(j)
    inside = bytearray(slots)
    for b in range(nkeys + 1):
        s, n = lay.start[b], lay.total[b]
        lo, hi = lay.pad[b]
        assert 0 <= s and s + n <= lay.npad and (lo == hi or (0 <= lo <= hi <= lay.npad))
        # 1. the bucket's slots hold exactly the bucket's caller indices, each once
        got = list(perm[s:s + n])
        assert sorted(got) == want[b], f"bucket {b}: perm[{s}:{s + n}] is not the bucket's jobs"
        for p in range(s, s + n):
            assert not inside[p], f"slot {p} belongs to two buckets"
            inside[p] = 1
            # 2. the job of the caller index perm names
            exp = expected_job(toks[perm[p]], base, cls_tab, nkeys)
            assert tuple(jobs[p]) == exp, f"slot {p} (job {perm[p]}, bucket {b}): {tuple(jobs[p])} != {exp}"
            # 4. verdict zeroed
            assert vpad[p] == 0, f"vpad[{p}] = {vpad[p]} on a filled slot"
        # 3. padding
        for p in range(lo, hi):
            assert not inside[p], f"slot {p} belongs to two buckets"
            inside[p] = 1
            assert tuple(jobs[p]) == pad_job(b, nkeys), f"pad slot {p} of bucket {b}: {tuple(jobs[p])}"
            assert perm[p] == -1, f"perm[{p}] = {perm[p]} on a pad slot"
            assert vpad[p] == 0, f"vpad[{p}] = {vpad[p]} on a pad slot"
        # 5. the cursor ran to the end of the bucket's jobs
        assert cursor[b] == s + n, f"cursor[{b}] = {cursor[b]}, want {s + n}"
    # 6. nothing outside the plan was written
    for p in range(slots):
        if inside[p]:
            continue
        bj, bp, bv = (JOB_SENT, PERM_SENT, BYTE_SENT) if before is None else (tuple(before[0][p]), before[1][p], before[2][p])
        assert tuple(jobs[p]) == bj and perm[p] == bp and vpad[p] == bv, f"slot {p} outside the plan was written"


def zc_stride(kmax):
    """bytes per slot of a key whose longest job spans kmax bytes (plan_chunk):
    up to 15 bytes in front of the job and 15 behind it, rounded to 16"""
    return (kmax + 30 + 15) & ~15


def gather_slot(job, p, kbase, kstart, kstride):
    """(d0, lo, hi): the slot's byte offset in dst and the aligned source span"""
    key = job_key(job)
    end = max(job[0] + job[1], job[2] + job_siglen(job))
    return kbase[key] + (p - kstart[key]) * kstride[key], job[0] & ~15, (end + 15) & ~15


def check_gather(src, jobs_in, begin, end, kbase, kstart, kstride, dst_len, jobs_out, dst):
    """src: the source bytes.  jobs_in: the npad jobs ahead of the gather.
    jobs_out: npad + GUARD jobs after it.  dst: GUARD + dst_len + GUARD bytes."""
    npad = len(jobs_in)
    assert len(jobs_out) == npad + GUARD and len(dst) == dst_len + 2 * GUARD
    may = bytearray(len(dst))                      # bytes inside some job's copied span
    for p in range(npad):
        jb, out = tuple(jobs_in[p]), tuple(jobs_out[p])
        if not (begin <= p < end and job_live(jb)):
            assert out == jb, f"job {p} is outside the gather and was rewritten: {out}"
            continue
        d0, lo, hi = gather_slot(jb, p, kbase, kstart, kstride)
        assert hi - lo <= kstride[job_key(jb)] and d0 + hi - lo <= dst_len, "the test's own layout is wrong"
        off, sig = d0 + (jb[0] - lo), d0 + (jb[2] - lo)
        assert out == (off, jb[1], sig, jb[3]), f"job {p}: {out}, want offsets {off}, {sig}"
        assert bytes(dst[GUARD + off:GUARD + off + jb[1]]) == bytes(src[jb[0]:jb[0] + jb[1]]), f"job {p}: signing input"
        n = job_siglen(jb)
        assert bytes(dst[GUARD + sig:GUARD + sig + n]) == bytes(src[jb[2]:jb[2] + n]), f"job {p}: signature"
        may[GUARD + d0:GUARD + d0 + hi - lo] = b"\1" * (hi - lo)
    for p in range(npad, npad + GUARD):
        assert tuple(jobs_out[p]) == JOB_SENT, f"guard job {p} was written"
    # every byte outside the copied spans is untouched (compared in runs, for speed)
    i, n = 0, len(dst)
    while i < n:
        k = may.find(1, i)
        k = n if k < 0 else k
        seg = bytes(dst[i:k])
        if seg != bytes([BYTE_SENT]) * (k - i):
            bad = next(q for q in range(k - i) if seg[q] != BYTE_SENT)
            raise AssertionError(f"dst byte {i + bad - GUARD} lies outside every copied span and was written")
        j = may.find(0, k)
        i = n if j < 0 else j


def check_scatter(perm, vpad, ntok, verdict):
    """verdict: GUARD + ntok + GUARD bytes; every perm entry >= 0 names a verdict once"""
    assert len(verdict) == ntok + 2 * GUARD
    want = [BYTE_SENT] * len(verdict)
    for p, t in enumerate(perm):
        if t >= 0:
            want[GUARD + t] = vpad[p]
    assert list(verdict) == want
