"""k_claims_match_each through the C ABI (jg_claims_match / Context.claims_match).
The reference is the host build (tests/host_unit/claims_match_test.cpp), byte
for byte: codes and masks.

* The whole CPU corpus (tests/claims_corpus.py) and the directed list of
  tests/claims_match_cases.py, packed at arena offsets 0..3 mod 4, under several
  predicate sets; the codes are jg_claims_each's.
* 1 / 63 / 64 / 65 / 4097 jobs with profile i % nexpect for nexpect 1, 2 and 64,
  both outputs poisoned, HOST masks zero, no poison left.
* One wave that mixes 3-character and 400-character segments, different
  profiles and nesting depths 1 to 6.
* Every -1 case and njobs == 0.
* The older entries give the same outputs before and after a match call: the
  kept device buffers are shared.
"""
import ctypes

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_each_cases as EC
from tests import claims_match_cases as MC
from tests import claims_paths_cases as PC
from tests import claims_select_cases as SC
from tests.test_gpu_claims_scan import EX, NOW, pack, sized_payload

pytestmark = pytest.mark.gpu

P = MC.P
OTHER = {"Issuer": "https://other.example/", "Audiences": ["www.example.com"]}     # sized_payload's issuer is wrong
POISON = 0xeeeeeeee
E, W, L, H = MC.EQUALS, MC.HAS_WORD, MC.HAS_ELEMENT, MC.PRESENT


def enc(paths):
    return [[c.encode() if isinstance(c, str) else bytes(c) for c in p] for p in paths]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The host build of claims_match_each: the reference of the device run."""
    d = tmp_path_factory.mktemp("claims_match_gpu")
    MC.build_host(str(d / "claims_match_test"))
    return d, str(d / "claims_match_test")


def host_run(host, name, sets, cases, reqs):
    """sets: resolved dicts; cases: (profile, segment) -> (codes, masks) of the host build"""
    d, exe = host
    path = str(d / (name + ".txt"))
    EC.write_sets(path, sets, cases)
    return MC.run_host(exe, path, reqs)


def device_run(ctx, arena, jobs, sets, reqs):
    paths, preds = MC.split(reqs)
    c, m = ctx.claims_match(arena, jobs, sets, enc(paths), preds)       # both outputs poisoned with 0xee
    assert len(c) == len(jobs) == len(m)
    return list(c), m


def assert_same(got, want, what=""):
    n = len(want[0])
    assert len(got[0]) == n and len(got[1]) == n, what
    diff = [k for k in range(n) if got[0][k] != want[0][k] or got[1][k] != want[1][k]]
    assert not diff, (what, [(k, got[0][k], want[0][k], hex(got[1][k]), hex(want[1][k])) for k in diff[:3]])


def assert_host_masks_zero(got, nreq):
    assert all(m == 0 for c, m in zip(*got) if c == _lib.CL_HOST)
    assert all(c <= _lib.CL_HOST for c in got[0])                        # no poison survives
    assert POISON not in got[1] and all(m >> nreq == 0 for m in got[1])


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
    codes = list(ctx.claims_each(arena, jobs, sets))
    for reqs in MC.CORPUS_SETS[1:]:
        got = device_run(ctx, arena, jobs, sets, reqs)
        assert_host_masks_zero(got, len(reqs))
        assert_same(got, host_run(host, "corpus%d" % g, sets, cases, reqs), "host build")
        assert got[0] == codes                                          # predicates change no decision


@pytest.mark.parametrize("lead", range(4))
def test_directed_list_at_every_alignment(ctx, host, lead):
    cases = MC.directed()
    sets = [CC.resolve(CC.FULL, cases[0][2]), CC.resolve({}, cases[0][2])]
    prof = [0 if ex else 1 for _, ex, _ in cases]
    segs = [seg for seg, _, _ in cases]
    arena, spans = pack(segs, lead=lead, gap=lead % 2)
    jobs = [(o, l, p) for (o, l), p in zip(spans, prof)]
    for reqs in MC.PRED_SETS:
        got = device_run(ctx, arena, jobs, sets, reqs)
        assert _lib.CL_HOST not in got[0]
        assert_same(got, host_run(host, "directed", sets, list(zip(prof, segs)), reqs), reqs)
        assert MC.check_masks(cases, got[0], got[1], reqs, no_host=True) == len(cases)


def pool_segments(n):
    C = CC.corpus()
    pool = C.plain + C.hard[:200] + [(c[0], 0) for c in MC.directed()] + [(c[0], 0) for c in SC.directed()]
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
        got = device_run(ctx, arena, jobs, sets, MC.FULL)
        assert_host_masks_zero(got, len(MC.FULL))
        want = host_run(host, "batch%d_%d" % (n, nexpect), sets, [(i % nexpect, s) for i, s in enumerate(segs)], MC.FULL)
        assert_same(got, want, "nexpect %d" % nexpect)


def nested(depth, k):
    """a payload that is valid at NOW for EX whose a/b/c/d chain is `depth` objects deep, over an array"""
    inner = b'["y%d","z"]' % k
    for key in (b"f", b"e", b"d", b"c", b"b", b"a")[6 - depth:]:
        inner = b'{"' + key + b'":' + inner + b',"x":[' + b'"z",' * (k % 5) + b"{}]}"
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
    reqs = tuple(MC.Elem(p, "z") for p in PC.PREFIXES) + tuple(MC.Has(p) for p in PC.PREFIXES) + (
        MC.Eq(P("iss"), "https://example.com/"), MC.Elem(P("a", "x"), "z"))
    got = device_run(ctx, arena, jobs, sets, reqs)
    assert_same(got, host_run(host, "wave", sets, list(zip(prof, segs)), reqs))
    assert got[0][0] == _lib.CL_NO_TIME and _lib.CL_HOST in got[0]
    assert {_lib.CL_OK, _lib.CL_ISS, _lib.CL_EXP} <= set(got[0])
    # every depth of the chain is reached in the wave: the array at a, a/b, a/b/c and a/b/c/d, and deeper than any path
    low = {m & 0xff for c, m in zip(*got) if c != _lib.CL_HOST}
    assert {0x11, 0x32, 0x74, 0xf8, 0xf0, 0x00} <= low


def test_bad_arguments_and_empty_batch(ctx):
    ex = CC.resolve(EX, NOW)
    ok_paths = [[b"a", b"b"], [b"c"]]
    ok = [(0, L, b"x"), (1, H, b"")]
    assert ctx.claims_match(b"", [], [ex], ok_paths, ok) == (b"", [])
    c, m = ctx.claims_match(b"e30", [(3, 0, 0), (0, 3, 1)], [ex, ex], ok_paths, ok)
    assert c == bytes([_lib.CL_HOST, _lib.CL_NO_TIME]) and m == [0, 0]
    c, m = ctx.claims_match(b"e30", [(0, 3, 0)], [ex], ok_paths, [])                # n == 0: every mask 0
    assert c == bytes([_lib.CL_NO_TIME]) and m == [0]
    c, m = ctx.claims_match(b"e30", [(0, 3, 0)], [ex], [], [])
    assert c == bytes([_lib.CL_NO_TIME]) and m == [0]
    one = [(0, 3, 0)]

    def refused(jobs, sets, paths=ok_paths, preds=ok, **kw):
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.claims_match(b"e30", jobs, sets, paths, preds, **kw)
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
    # everything jg_claims_paths refuses
    refused(one, [ex], [[b"n%d" % k] for k in range(9)], [])      # more than JG_MAX_PATHS
    refused(one, [ex], [[]], [])                                  # no component
    refused(one, [ex], [[b"a", b"b", b"c", b"d", b"e"]], [])      # more than JG_PATH_MAX_COMP
    for comp in (b"", b"L" * 65, b"a\x1fb", b"a\x7fb", b"a\x80b", b'a"b', b"a\\b", b"a\x00b"):
        refused(one, [ex], [[b"a", comp]], [])
    refused(one, [ex], [[b"a", b"b"], [b"a", b"b"]], [])          # two equal paths
    # the predicates
    refused(one, [ex], preds=[(k % 2, L, b"v%d" % k) for k in range(17)])       # more than JG_MAX_PRED
    refused(one, [ex], preds=[(2, E, b"x")])                      # a path index past the paths
    refused(one, [ex], preds=[(255, H, b"")])
    refused(one, [ex], [], [(0, H, b"")])
    for op in (0, 5, 255):                                        # an unknown op
        refused(one, [ex], preds=[(0, op, b"x")])
    for op, v in ((E, b"v" * 65), (W, b""), (W, b"v" * 65), (L, b""), (L, b"v" * 65), (H, b"x")):    # a length outside the op's range
        refused(one, [ex], preds=[(0, op, v)])
    for v in (b"a\x1fb", b"a\x7fb", b"a\x80b", b"\xc3\xa9", b'a"b', b"a\\b", b"a\x00b"):               # a refused value byte
        for op in (E, W, L):
            refused(one, [ex], preds=[(1, op, v)])
    refused(one, [ex], preds=[(0, W, b"a b")])                    # a space in a HAS_WORD value
    refused(one, [ex], preds=[(0, E, b"x"), (1, E, b"x"), (0, E, b"x")])        # two identical predicates
    refused(one, [ex], preds=[(1, H, b""), (1, H, b"")])
    for null in ("paths", "preds", "codes", "masks"):             # a NULL with jobs
        refused(one, [ex], null=(null,))
    assert ctx.claims_match(b"", [], [ex], ok_paths, ok, null=("paths", "preds", "codes", "masks")) == (b"", [])    # njobs == 0
    # the limits themselves are taken
    c, m = ctx.claims_match(b"e30", one, [ex] * 64, [[b"L" * 64] * 4] + [[b"n%d" % k, b"x"] for k in range(7)],
                            [(k % 8, (E, W, L)[k % 3], b"v" * 64) for k in range(15)] + [(0, E, b"")])
    assert c == bytes([_lib.CL_NO_TIME]) and m == [0]
    # every output unwritten at -1
    lib = _lib.lib()
    job = (_lib.JgCJob * 1)()
    job[0].off, job[0].len, job[0].flags = 0, 3, 0
    e = _lib.JgExpect()
    e.now_sec = CC.T0
    keep = ctypes.create_string_buffer(b"ab", 2)
    ps = _lib.JgPaths()
    ps.names, ps.n = ctypes.cast(keep, ctypes.c_void_p), 1
    ps.ncomp[0] = 2
    ps.comp_len[0][0] = ps.comp_len[0][1] = 1
    vkeep = ctypes.create_string_buffer(b"x", 1)
    qs = _lib.JgPreds()
    qs.values, qs.n = ctypes.cast(vkeep, ctypes.c_void_p), 1
    qs.path[0], qs.op[0], qs.value_len[0] = 0, L, 1

    def raw_call(ncomp=2, flags=0, nexpect=1, op=L, path=0):
        ps.ncomp[0] = ncomp
        job[0].flags = flags
        qs.op[0], qs.path[0] = op, path
        out = ctypes.create_string_buffer(b"\xee", 1)
        m = ctypes.create_string_buffer(b"\xee" * 4, 4)
        rc = lib.jg_claims_match(ctx.h, b"e30", 3, job, 1, ctypes.byref(e), nexpect, ctypes.byref(ps), ctypes.byref(qs),
                                 out, ctypes.cast(m, ctypes.c_void_p))
        return rc, out.raw + m.raw
    untouched = b"\xee" * 5
    assert raw_call(ncomp=0) == (-1, untouched)
    assert raw_call(flags=1) == (-1, untouched)
    assert raw_call(nexpect=65) == (-1, untouched)
    assert raw_call(op=9) == (-1, untouched)
    assert raw_call(path=1) == (-1, untouched)
    assert "jg_claims_match" in ctx.error() and "predicates" in ctx.error()
    assert raw_call() == (0, bytes([_lib.CL_NO_TIME]) + bytes(4))
    # then a good call on the same context
    seg = CC.b64(b'{"cnf":{"jkt":"a"},"scope":"x read","exp":%d}' % (CC.T0 + 600))
    codes, masks = ctx.claims_match(seg, [(0, len(seg), 1)], [CC.resolve({}, NOW), ex], [[b"cnf", b"nope"], [b"cnf", b"jkt"], [b"scope"]],
                                    [(0, H, b""), (1, E, b"a"), (2, W, b"read"), (2, W, b"rea"), (1, H, b"")])
    assert codes == bytes([_lib.CL_ISS]) and masks == [0b10110]


def test_old_entries_unchanged_around_a_match_call(ctx):
    segs = pool_segments(300)
    arena, spans = pack(segs, lead=2)
    sets = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW)]
    jobs = [(o, l, i % 2) for i, (o, l) in enumerate(spans)]
    names = [n.encode() for n in SC.EIGHT]

    def old():
        a = ctx.claims_each(arena, jobs, sets, mode="select", names=names)
        b = ctx.claims_paths(arena, jobs, sets, enc(PC.EIGHT))
        return (a[0], bytes(a[1]), bytes(a[2]), b[0], bytes(b[1]), bytes(b[2]),
                ctx.claims_scan(arena, spans, sets[1]), bytes(ctx.claims_extract(arena, spans, sets[0])[1]))
    before = old()
    # a smaller batch with other paths in between: the kept buffers are shared
    small = device_run(ctx, arena, jobs[:70], sets, MC.CORPUS_SETS[1])
    assert old() == before
    assert device_run(ctx, arena, jobs[:70], sets, MC.CORPUS_SETS[1]) == small
    assert small[0] == list(before[0][:70])
    assert len(set(before[0])) >= 5 and any(small[1])
