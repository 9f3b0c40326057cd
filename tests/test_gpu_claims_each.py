"""k_claims_scan_each / k_claims_extract_each / k_claims_select_each through the C
ABI (jg_claims_each / Context.claims_each).  The references are the host build
(tests/host_unit/claims_each_test.cpp) and the existing single-profile entries
called once per Expected set, byte for byte.

* The whole CPU corpus (tests/claims_corpus.py) in three calls of at most 64
  profiles, the jobs ordered so that neighbouring lanes hold different profiles,
  in all three modes.
* nexpect == 1 is jg_claims_scan / _extract / _select on the same jobs.
* 1 / 63 / 64 / 65 / 4097 jobs with profile i % nexpect for nexpect 1, 2 and 64,
  all outputs poisoned, HOST records zero.
* A wave that mixes 3-character and 400-character segments of different
  profiles; every segment length at every offset mod 4 with the last job ending
  at arena_len; a table filled to the last byte of its pool.
* Every -1 case, njobs == 0, and the old entries still refusing nonzero flags.
"""
import ctypes

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_each_cases as EC
from tests import claims_select_cases as SC
from tests.test_gpu_claims_scan import EX, NOW, pack, sized_payload

pytestmark = pytest.mark.gpu

NAMES = EC.NAMES
OTHER = {"Issuer": "https://other.example/", "Audiences": ["www.example.com"]}     # sized_payload's issuer is wrong
LATE = dict(EX)                                                                   # EX at a clock where everything is over


def enc(names):
    return [n.encode() if isinstance(n, str) else n for n in names]


def split(raw, size):
    raw = bytes(raw)
    return [raw[size * k:size * k + size] for k in range(len(raw) // size)]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The host build of the *_each functions: the reference of the device run."""
    d = tmp_path_factory.mktemp("claims_each_gpu")
    EC.build_host(str(d / "claims_each_test"))
    CC.write_cases(str(d / "cases.txt"))
    return d, str(d / "claims_each_test")


def host_run(host, name, sets, cases, names=NAMES):
    """sets: resolved dicts; cases: (profile, segment) -> (codes, records, selected) lists of the host build"""
    d, exe = host
    path = str(d / (name + ".txt"))
    EC.write_sets(path, sets, cases)
    dec, (xc, xr), (sc, sr, sq) = EC.run_host(exe, path, 0, len(sets), names)
    assert dec == xc == sc and xr == sr
    return sc, sr, sq


def device_run(ctx, arena, jobs, sets, names=NAMES):
    """all three modes of one batch -> (codes, records, selected) lists; the modes agree"""
    c0 = ctx.claims_each(arena, jobs, sets)
    c1, v1 = ctx.claims_each(arena, jobs, sets, mode="extract")
    c2, v2, q2 = ctx.claims_each(arena, jobs, sets, mode="select", names=enc(names))
    assert c0 == c1 == c2 and bytes(v1) == bytes(v2)
    assert len(c0) == len(jobs)
    return list(c2), split(v2, 64), split(q2, 80)


def assert_same(got, want, what=""):
    n = len(want[0])
    assert all(len(g) == n for g in got), what
    diff = [k for k in range(n) if any(got[j][k] != want[j][k] for j in range(3))]
    assert not diff, (what, [(k, got[0][k], want[0][k], got[1][k].hex(), want[1][k].hex(), got[2][k].hex(),
                              want[2][k].hex()) for k in diff[:3]])


def assert_host_records_zero(got):
    assert all(r == bytes(64) and q == bytes(80) for c, r, q in zip(*got) if c == _lib.CL_HOST)
    assert b"\xee" * 64 not in got[1] and not any(b"\xee" * 4 in q for q in got[2])      # no poison survives
    assert all(c <= _lib.CL_HOST for c in got[0])


@pytest.mark.parametrize("g", range(3))
def test_corpus_equals_host_build_and_single_profile_entries(ctx, host, g):
    C = CC.corpus()
    lo, hi = EC.groups()[g]
    allc = C.all_cases()
    idx = EC.group_cases(lo, hi)
    # round-robin over the sets: neighbouring jobs hold different profiles
    rank, seen = {}, {}
    for k in idx:
        si = allc[k][1]
        rank[k] = seen.get(si, 0)
        seen[si] = rank[k] + 1
    order = sorted(idx, key=lambda k: (rank[k], allc[k][1]))
    assert sum(1 for a, b in zip(order, order[1:]) if allc[a][1] != allc[b][1]) > 0.8 * len(order)
    arena, spans = pack([allc[k][0] for k in order], lead=g + 1, gap=1)
    sets = [CC.resolve(*C.sets[si]) for si in range(lo, hi)]
    jobs = [(off, ln, allc[k][1] - lo) for k, (off, ln) in zip(order, spans)]
    got = device_run(ctx, arena, jobs, sets)
    assert_host_records_zero(got)
    # the host build prints the group in all_cases() order
    d, exe = host
    dec, (xc, xr), (sc, sr, sq) = EC.run_host(exe, str(d / "cases.txt"), lo, hi, NAMES)
    at = {k: j for j, k in enumerate(idx)}
    want = ([sc[at[k]] for k in order], [sr[at[k]] for k in order], [sq[at[k]] for k in order])
    assert dec == xc == sc
    assert_same(got, want, "host build")
    # the single-profile entries, one call per set on the same arena
    for si in range(lo, hi):
        js = [j for j, k in enumerate(order) if allc[k][1] == si]
        sp = [spans[j] for j in js]
        ex = sets[si - lo]
        c, v, q = ctx.claims_select(arena, sp, ex, enc(NAMES))
        one = (list(c), split(v, 64), split(q, 80))
        assert_same(tuple([x[j] for j in js] for x in got), one, "set %d" % si)
        assert ctx.claims_scan(arena, sp, ex) == c
        xc1, xv1 = ctx.claims_extract(arena, sp, ex)
        assert xc1 == c and bytes(xv1) == bytes(v)


def pool_segments(n):
    C = CC.corpus()
    pool = C.plain + C.hard[:200] + [(c[0], 0) for c in SC.directed()]
    return [pool[(7 * k) % len(pool)][0] for k in range(n)]


def test_one_profile_is_the_old_entries(ctx):
    segs = pool_segments(700)
    arena, spans = pack(segs, lead=1)
    ex = CC.resolve(EX, NOW)
    jobs = [(o, l, 0) for o, l in spans]
    got = device_run(ctx, arena, jobs, [ex])
    c, v, q = ctx.claims_select(arena, spans, ex, enc(NAMES))
    assert_same(got, (list(c), split(v, 64), split(q, 80)))
    assert ctx.claims_scan(arena, spans, ex) == bytes(got[0])
    assert len(set(got[0])) >= 5


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes_and_profile_counts(ctx, host, n):
    C = CC.corpus()
    all_sets = [CC.resolve(*C.sets[si]) for si in range(3, 67)]        # 64 sets with strings
    segs = pool_segments(n)
    arena, spans = pack(segs, lead=3)
    for nexpect in (1, 2, 64):
        sets = all_sets[:nexpect]
        jobs = [(o, l, i % nexpect) for i, (o, l) in enumerate(spans)]
        got = device_run(ctx, arena, jobs, sets, SC.EIGHT)             # all outputs poisoned with 0xee
        assert_host_records_zero(got)
        want = host_run(host, "batch%d_%d" % (n, nexpect), sets, [(i % nexpect, s) for i, s in enumerate(segs)],
                        SC.EIGHT)
        assert_same(got, want, "nexpect %d" % nexpect)


def test_wave_mixing_short_and_long_segments_of_different_profiles(ctx, host):
    long = [CC.b64(sized_payload(400, k)) for k in range(2)]
    segs = [b"e30", long[0], b"e30", long[1]] * 16 + [b"e3", long[0], b"e30"]
    sets = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW), CC.resolve(LATE, NOW + 7200 * CC.SECOND)]
    prof = [i % 3 if i % 2 == 0 else (1, 2, 0)[(i // 4) % 3] for i in range(len(segs))]
    arena, spans = pack(segs)
    jobs = [(o, l, p) for (o, l), p in zip(spans, prof)]
    got = device_run(ctx, arena, jobs, sets)
    assert_same(got, host_run(host, "wave", sets, list(zip(prof, segs))))
    assert got[0][0] == _lib.CL_NO_TIME and got[0][64] == _lib.CL_HOST
    # the same long segment under the three profiles: wrong issuer, accepted, expired
    assert (prof[1], prof[9], prof[5]) == (1, 0, 2) and segs[1] == segs[9] == segs[5]
    assert (got[0][1], got[0][9], got[0][5]) == (_lib.CL_ISS, _lib.CL_OK, _lib.CL_EXP)
    assert got[1][1] == got[1][9] == got[1][5] != bytes(64)             # the records do not depend on the profile


def test_every_length_and_alignment(ctx, host):
    """Segments of every length 0..400 at every offset mod 4, the last job ending
    at arena_len, the profile changing from job to job."""
    long = CC.b64(sized_payload(400))
    segs = [CC.b64(sized_payload(n, n)) if n >= 136 and n % 4 != 1 else long[:n] for n in range(401)]
    assert [len(s) for s in segs] == list(range(401))
    sets = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW), CC.resolve(LATE, NOW + 7200 * CC.SECOND)]
    prof = [n % 3 for n in range(401)]
    want = host_run(host, "lengths", sets, list(zip(prof, segs)))
    assert {_lib.CL_OK, _lib.CL_ISS, _lib.CL_EXP, _lib.CL_HOST} <= set(want[0])
    for lead in range(4):
        arena, spans = pack(segs, lead=lead)
        assert spans[-1][0] + spans[-1][1] == len(arena) and {o % 4 for o, _ in spans} == {0, 1, 2, 3}
        got = device_run(ctx, arena, [(o, l, p) for (o, l), p in zip(spans, prof)], sets)
        assert_same(got, want, "lead %d" % lead)


def test_full_pool_table(ctx, host):
    sets, cases, want = EC.full_pool()
    arena, spans = pack([seg for _, seg in cases], lead=2, gap=3)
    jobs = [(o, l, si) for (o, l), (si, _) in zip(spans, cases)]
    got = device_run(ctx, arena, jobs, sets, ("aud",))
    assert got[0] == want
    assert_same(got, host_run(host, "full", sets, cases, ("aud",)))
    # a smaller table after the full one sees nothing of it
    ex = CC.resolve(EX, NOW)
    seg = CC.b64(sized_payload(200))
    assert ctx.claims_each(seg, [(0, len(seg), 0)], [ex]) == bytes([_lib.CL_OK])


def test_bad_arguments_and_empty_batch(ctx):
    ex = CC.resolve(EX, NOW)
    assert ctx.claims_each(b"", [], [ex]) == b""
    assert ctx.claims_each(b"e30", [(3, 0, 0), (0, 3, 1)], [ex, ex]) == bytes([_lib.CL_HOST, _lib.CL_NO_TIME])
    one = [(0, 3, 0)]

    def refused(jobs, sets, **kw):
        for mode in ("scan", "extract", "select"):
            with pytest.raises(_lib.JgError, match="rc=-1"):
                ctx.claims_each(b"e30", jobs, sets, mode=mode, names=[b"scope"] if mode == "select" else None, **kw)
    refused(one, [])                                              # nexpect == 0
    refused(one, [ex], nexpect=0)
    refused(one, [ex] * 65)                                       # more than JG_MAX_PROFILES
    assert ctx.claims_each(b"e30", one, [ex] * 64) == bytes([_lib.CL_NO_TIME])
    refused([(0, 3, 1)], [ex])                                    # flags >= nexpect
    refused([(0, 3, 0), (0, 3, 2)], [ex, ex])
    refused([(0, 3, 0xffffffff)], [ex])
    refused(one, [ex, dict(ex, audiences=[b"a"] * 17)])           # a profile jg_claims_scan refuses
    refused(one, [dict(ex, now_nsec=10**9), ex])
    refused(one, [dict(ex, issuer=b"i" * 4097)])
    fat = dict(ex, issuer=b"i" * 2731, audiences=[])
    refused(one, [fat, fat, dict(fat, issuer=b"i" * 2731)])       # 8193 bytes in all
    assert ctx.claims_each(b"e30", one, [fat, fat, dict(fat, issuer=b"i" * 2730)]) == bytes([_lib.CL_NO_TIME])
    for jobs in ([(0, 4, 0)], [(4, 0, 0)], [(2, 2, 0)], [(0, 3, 0), (1 << 40, 1, 0)]):    # a span past arena_len
        refused(jobs, [ex])
    with pytest.raises(_lib.JgError, match="rc=-1"):               # a select jg_claims_select refuses
        ctx.claims_each(b"e30", one, [ex], mode="select", names=[b"x", b"x"])
    # the NULL combinations, and every output unwritten at -1
    L = _lib.lib()
    job = (_lib.JgCJob * 1)()
    job[0].off, job[0].len, job[0].flags = 0, 3, 0
    e = _lib.JgExpect()
    e.now_sec = CC.T0
    keep = ctypes.create_string_buffer(b"scope", 5)
    s = _lib.JgSelect()
    s.names, s.n = ctypes.cast(keep, ctypes.c_void_p), 1
    s.name_len[0] = 5

    def raw_call(expects=True, nexpect=1, select=False, code=True, vals=False, sels=False, njobs=1, flags=0):
        job[0].flags = flags
        out = ctypes.create_string_buffer(b"\xee", 1)
        v = ctypes.create_string_buffer(b"\xee" * 64, 64)
        q = ctypes.create_string_buffer(b"\xee" * 80, 80)
        rc = L.jg_claims_each(ctx.h, b"e30", 3, job, njobs, ctypes.byref(e) if expects else None, nexpect,
                              ctypes.byref(s) if select else None, out if code else None,
                              ctypes.cast(v, ctypes.c_void_p) if vals else None,
                              ctypes.cast(q, ctypes.c_void_p) if sels else None)
        return rc, out.raw + v.raw + q.raw
    untouched = b"\xee" * 145
    assert raw_call(sels=True, vals=True) == (-1, untouched)              # sel_out without select
    assert raw_call(sels=True, select=True) == (-1, untouched)            # sel_out without vals_out
    assert raw_call(expects=False) == (-1, untouched)
    assert raw_call(code=False) == (-1, untouched)
    assert raw_call(nexpect=0) == (-1, untouched)
    assert raw_call(nexpect=65) == (-1, untouched)
    assert raw_call(flags=1) == (-1, untouched)
    assert raw_call(flags=1, vals=True) == (-1, untouched)
    assert raw_call(code=False, njobs=0) == (0, untouched)                # njobs == 0
    # the three modes by their outputs; `select` without sel_out is not looked at
    assert raw_call() == (0, bytes([_lib.CL_NO_TIME]) + untouched[1:])
    assert raw_call(vals=True, select=True) == (0, bytes([_lib.CL_NO_TIME]) + bytes(64) + b"\xee" * 80)
    assert raw_call(vals=True, select=True, sels=True) == (0, bytes([_lib.CL_NO_TIME]) + bytes(144))
    # then a good call on the same context
    seg = CC.b64(b'{"scope":"a","exp":%d}' % (CC.T0 + 600))
    codes, vals, sel = ctx.claims_each(seg, [(0, len(seg), 1)], [CC.resolve({}, NOW), ex], mode="select",
                                       names=[b"nope", b"scope"])
    assert codes == bytes([_lib.CL_ISS])
    assert (sel[0].off[1], sel[0].len[1], sel[0].type[1], sel[0].type[0]) == (10, 1, _lib.SEL_STRING, _lib.SEL_ABSENT)


def test_old_entries_still_refuse_nonzero_flags(ctx):
    ex = CC.resolve(EX, NOW)
    for flags in (1, 63):
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.claims_scan(b"e30", [(0, 3)], ex, flags=flags)
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.claims_extract(b"e30", [(0, 3)], ex, flags=flags)
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.claims_select(b"e30", [(0, 3)], ex, [b"scope"], flags=flags)
    assert ctx.claims_scan(b"e30", [(0, 3)], ex) == bytes([_lib.CL_NO_TIME])
