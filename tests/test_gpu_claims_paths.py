"""k_claims_paths_each through the C ABI (jg_claims_paths / Context.claims_paths).
The reference is the host build (tests/host_unit/claims_paths_test.cpp), byte
for byte: codes, jg_claims and jg_selected records.

* The whole CPU corpus (tests/claims_corpus.py) and the directed list of
  tests/claims_paths_cases.py, packed at arena offsets 0..3 mod 4, under several
  path sets; codes and jg_claims are jg_claims_each's.
* 1 / 63 / 64 / 65 / 4097 jobs with profile i % nexpect for nexpect 1, 2 and 64,
  all outputs poisoned, HOST records zero.
* One wave that mixes 3-character and 400-character segments, different
  profiles and nesting depths 1 to 6.
* Every -1 case and njobs == 0.
* The old entries give the same outputs before and after a paths call: the kept
  device buffers are shared.
"""
import ctypes

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_each_cases as EC
from tests import claims_paths_cases as PC
from tests import claims_select_cases as SC
from tests.test_gpu_claims_scan import EX, NOW, pack, sized_payload

pytestmark = pytest.mark.gpu

P = PC.P
OTHER = {"Issuer": "https://other.example/", "Audiences": ["www.example.com"]}     # sized_payload's issuer is wrong
CORPUS_PATHS = PC.CORPUS_SETS[3]


def enc(paths):
    return [[c.encode() if isinstance(c, str) else bytes(c) for c in p] for p in paths]


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
    """The host build of claims_paths_each: the reference of the device run."""
    d = tmp_path_factory.mktemp("claims_paths_gpu")
    PC.build_host(str(d / "claims_paths_test"))
    return d, str(d / "claims_paths_test")


def host_run(host, name, sets, cases, paths):
    """sets: resolved dicts; cases: (profile, segment) -> (codes, records, selected) lists of the host build"""
    d, exe = host
    path = str(d / (name + ".txt"))
    EC.write_sets(path, sets, cases)
    return PC.run_host(exe, path, paths)


def device_run(ctx, arena, jobs, sets, paths):
    c, v, q = ctx.claims_paths(arena, jobs, sets, enc(paths))       # all outputs poisoned with 0xee
    assert len(c) == len(jobs)
    return list(c), split(v, 64), split(q, 80)


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
def test_corpus_equals_host_build(ctx, host, g):
    C = CC.corpus()
    lo, hi = EC.groups()[g]
    allc = C.all_cases()
    idx = EC.group_cases(lo, hi)
    sets = [CC.resolve(*C.sets[si]) for si in range(lo, hi)]
    cases = [(allc[k][1] - lo, allc[k][0]) for k in idx]
    arena, spans = pack([seg for _, seg in cases], lead=g + 1, gap=1)
    assert {o % 4 for o, _ in spans} == {0, 1, 2, 3}
    jobs = [(o, l, p) for (o, l), (p, _) in zip(spans, cases)]
    for paths in (CORPUS_PATHS, PC.CORPUS_SETS[2]):
        got = device_run(ctx, arena, jobs, sets, paths)
        assert_host_records_zero(got)
        assert_same(got, host_run(host, "corpus%d" % g, sets, cases, paths), "host build")
        # selecting by path changes no decision and no jg_claims record
        c, v = ctx.claims_each(arena, jobs, sets, mode="extract")
        assert (list(c), split(v, 64)) == got[:2]


@pytest.mark.parametrize("lead", range(4))
def test_directed_list_at_every_alignment(ctx, host, lead):
    cases = PC.directed()
    sets = [CC.resolve(CC.FULL, cases[0][2]), CC.resolve({}, cases[0][2])]
    prof = [0 if ex else 1 for _, ex, _ in cases]
    segs = [seg for seg, _, _ in cases]
    arena, spans = pack(segs, lead=lead, gap=lead % 2)
    jobs = [(o, l, p) for (o, l), p in zip(spans, prof)]
    for paths in PC.PATH_SETS:
        got = device_run(ctx, arena, jobs, sets, paths)
        assert _lib.CL_HOST not in got[0]
        assert_same(got, host_run(host, "directed", sets, list(zip(prof, segs)), paths), paths)
        assert PC.check_selected(cases, got[0], got[2], paths, no_host=True) == len(cases)


def test_one_component_paths_are_jg_claims_selects_records(ctx):
    segs = pool_segments(700)
    arena, spans = pack(segs, lead=1)
    ex = CC.resolve(EX, NOW)
    got = device_run(ctx, arena, [(o, l, 0) for o, l in spans], [ex], [P(n) for n in SC.EIGHT])
    c, v, q = ctx.claims_select(arena, spans, ex, [n.encode() for n in SC.EIGHT])
    assert_same(got, (list(c), split(v, 64), split(q, 80)))


def pool_segments(n):
    C = CC.corpus()
    pool = C.plain + C.hard[:200] + [(c[0], 0) for c in PC.directed()] + [(c[0], 0) for c in SC.directed()]
    return [pool[(7 * k) % len(pool)][0] for k in range(n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes_and_profile_counts(ctx, host, n):
    C = CC.corpus()
    all_sets = [CC.resolve(*C.sets[si]) for si in range(3, 67)]        # 64 sets with strings
    segs = pool_segments(n)
    arena, spans = pack(segs, lead=3)
    for nexpect in (1, 2, 64):
        sets = all_sets[:nexpect]
        jobs = [(o, l, i % nexpect) for i, (o, l) in enumerate(spans)]
        got = device_run(ctx, arena, jobs, sets, PC.EIGHT)
        assert_host_records_zero(got)
        want = host_run(host, "batch%d_%d" % (n, nexpect), sets, [(i % nexpect, s) for i, s in enumerate(segs)], PC.EIGHT)
        assert_same(got, want, "nexpect %d" % nexpect)


def nested(depth, k):
    """a payload that is valid at NOW for EX whose a/b/c/d chain is `depth` objects deep"""
    inner = b"%d" % k
    for key in (b"f", b"e", b"d", b"c", b"b", b"a")[6 - depth:]:
        inner = b'{"' + key + b'":' + inner + b',"x":[' + b"1," * (k % 5) + b"{}]}"
    return b'{"exp":%d,"iss":"https://example.com/","aud":"www.example.com",' % (CC.T0 + 600) + inner[1:]


def test_wave_mixing_lengths_profiles_and_depths(ctx, host):
    long = [CC.b64(sized_payload(400, k)) for k in range(2)]
    deep = [CC.b64(nested(1 + k % 6, k)) for k in range(12)]
    segs = [b"e30", long[0], deep[0], long[1]] * 4 + deep + [b"e30", deep[5]] * 16 + [b"e3", long[0], deep[11], deep[4]]
    assert len(segs) == 64                                              # one wave
    sets = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW), CC.resolve(EX, NOW + 7200 * CC.SECOND)]
    prof = [i % 3 for i in range(len(segs))]
    arena, spans = pack(segs)
    jobs = [(o, l, p) for (o, l), p in zip(spans, prof)]
    got = device_run(ctx, arena, jobs, sets, PC.PREFIXES)
    assert_same(got, host_run(host, "wave", sets, list(zip(prof, segs)), PC.PREFIXES))
    assert got[0][0] == _lib.CL_NO_TIME and _lib.CL_HOST in got[0]
    assert {_lib.CL_OK, _lib.CL_ISS, _lib.CL_EXP} <= set(got[0])
    # every depth of the chain is reached in the wave: a/b/c/d filled, and absent where the chain is shorter
    types = {tuple(SC.unpack(q)["type"][:4]) for c, q in zip(got[0], got[2]) if c != _lib.CL_HOST}
    O, N, A = _lib.SEL_OBJECT, _lib.SEL_NUMBER, _lib.SEL_ABSENT
    assert {(N, A, A, A), (O, N, A, A), (O, O, N, A), (O, O, O, N), (O, O, O, O), (A, A, A, A)} <= types


def test_bad_arguments_and_empty_batch(ctx):
    ex = CC.resolve(EX, NOW)
    ok = [[b"a", b"b"]]
    assert ctx.claims_paths(b"", [], [ex], ok)[0] == b""
    c, v, q = ctx.claims_paths(b"e30", [(3, 0, 0), (0, 3, 1)], [ex, ex], ok)
    assert c == bytes([_lib.CL_HOST, _lib.CL_NO_TIME]) and bytes(q) == bytes(160)
    c, v, q = ctx.claims_paths(b"e30", [(0, 3, 0)], [ex], [])                     # n == 0: all ABSENT
    assert c == bytes([_lib.CL_NO_TIME]) and bytes(q) == bytes(80)
    one = [(0, 3, 0)]

    def refused(jobs, sets, paths=ok, **kw):
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.claims_paths(b"e30", jobs, sets, paths, **kw)
    # everything jg_claims_each refuses
    refused(one, [])
    refused(one, [ex], nexpect=0)
    refused(one, [ex] * 65)
    refused([(0, 3, 1)], [ex])                                    # flags >= nexpect
    refused([(0, 3, 0xffffffff)], [ex])
    refused(one, [ex, dict(ex, audiences=[b"a"] * 17)])
    refused(one, [dict(ex, now_nsec=10**9), ex])
    refused(one, [dict(ex, issuer=b"i" * 4097)])
    for jobs in ([(0, 4, 0)], [(4, 0, 0)], [(2, 2, 0)], [(0, 3, 0), (1 << 40, 1, 0)]):    # a span past arena_len
        refused(jobs, [ex])
    # the paths
    refused(one, [ex], [[b"n%d" % k] for k in range(9)])          # more than JG_MAX_PATHS
    refused(one, [ex], [[]])                                      # no component
    refused(one, [ex], [[b"a"], []])
    refused(one, [ex], [[b"a", b"b", b"c", b"d", b"e"]])          # more than JG_PATH_MAX_COMP
    for comp in (b"", b"L" * 65, b"a\x1fb", b"a\x7fb", b"a\x80b", b'a"b', b"a\\b", b"a\x00b"):
        refused(one, [ex], [[b"a", comp]])
        refused(one, [ex], [[comp]])
    refused(one, [ex], [[b"a", b"b"], [b"a", b"b"]])              # two equal paths
    refused(one, [ex], [[b"a"], [b"b", b"c"], [b"a"]])
    for null in ("paths", "vals", "sels"):                        # a NULL with jobs
        refused(one, [ex], null=(null,))
    assert ctx.claims_paths(b"", [], [ex], ok, null=("paths", "vals", "sels"))[0] == b""    # njobs == 0
    # the limits themselves are taken
    c, _, q = ctx.claims_paths(b"e30", one, [ex] * 64, [[b"L" * 64] * 4] + [[b"n%d" % k, b"x"] for k in range(7)])
    assert c == bytes([_lib.CL_NO_TIME]) and bytes(q) == bytes(80)
    # every output unwritten at -1
    L = _lib.lib()
    job = (_lib.JgCJob * 1)()
    job[0].off, job[0].len, job[0].flags = 0, 3, 0
    e = _lib.JgExpect()
    e.now_sec = CC.T0
    keep = ctypes.create_string_buffer(b"ab", 2)
    ps = _lib.JgPaths()
    ps.names, ps.n = ctypes.cast(keep, ctypes.c_void_p), 1
    ps.ncomp[0] = 2
    ps.comp_len[0][0] = ps.comp_len[0][1] = 1

    def raw_call(ncomp=2, flags=0, nexpect=1):
        ps.ncomp[0] = ncomp
        job[0].flags = flags
        out = ctypes.create_string_buffer(b"\xee", 1)
        v = ctypes.create_string_buffer(b"\xee" * 64, 64)
        q = ctypes.create_string_buffer(b"\xee" * 80, 80)
        rc = L.jg_claims_paths(ctx.h, b"e30", 3, job, 1, ctypes.byref(e), nexpect, ctypes.byref(ps), out,
                               ctypes.cast(v, ctypes.c_void_p), ctypes.cast(q, ctypes.c_void_p))
        return rc, out.raw + v.raw + q.raw
    untouched = b"\xee" * 145
    assert raw_call(ncomp=0) == (-1, untouched)
    assert raw_call(ncomp=5) == (-1, untouched)
    assert raw_call(flags=1) == (-1, untouched)
    assert raw_call(nexpect=65) == (-1, untouched)
    assert raw_call() == (0, bytes([_lib.CL_NO_TIME]) + bytes(144))
    # then a good call on the same context
    seg = CC.b64(b'{"cnf":{"jkt":"a"},"exp":%d}' % (CC.T0 + 600))
    codes, vals, sel = ctx.claims_paths(seg, [(0, len(seg), 1)], [CC.resolve({}, NOW), ex], [[b"cnf", b"nope"], [b"cnf", b"jkt"]])
    assert codes == bytes([_lib.CL_ISS])
    assert (sel[0].off[1], sel[0].len[1], sel[0].type[1], sel[0].type[0]) == (15, 1, _lib.SEL_STRING, _lib.SEL_ABSENT)


def test_old_entries_unchanged_around_a_paths_call(ctx):
    segs = pool_segments(300)
    arena, spans = pack(segs, lead=2)
    sets = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW)]
    jobs = [(o, l, i % 2) for i, (o, l) in enumerate(spans)]
    names = [n.encode() for n in SC.EIGHT]

    def old():
        a = ctx.claims_each(arena, jobs, sets, mode="select", names=names)
        b = ctx.claims_select(arena, spans, sets[0], names)
        return (a[0], bytes(a[1]), bytes(a[2]), b[0], bytes(b[1]), bytes(b[2]),
                ctx.claims_scan(arena, spans, sets[1]), bytes(ctx.claims_extract(arena, spans, sets[0])[1]))
    before = old()
    # a smaller batch with other paths in between: the kept buffers are shared
    small = ctx.claims_paths(arena, jobs[:70], sets, enc(PC.EIGHT))
    assert old() == before
    again = ctx.claims_paths(arena, jobs[:70], sets, enc(PC.EIGHT))
    assert (small[0], bytes(small[1]), bytes(small[2])) == (again[0], bytes(again[1]), bytes(again[2]))
    assert len(set(before[0])) >= 5
