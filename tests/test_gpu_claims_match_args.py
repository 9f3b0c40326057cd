"""k_claims_match_args through the C ABI (jg_claims_match_args /
Context.claims_match_args).  The reference is the host build of the same code
(tests/host_unit/claims_match_args_test.cpp), byte for byte: codes and masks.

* The whole CPU corpus (tests/claims_corpus.py) with operands derived from the
  token index, under a string and a numeric predicate set.
* The directed list of tests/claims_match_args_cases.py with its own operands at
  payload lead 0..3 x operand offset 0..3; the last operand ends at the last byte
  of the operand bytes.
* 1 / 63 / 64 / 65 / 257 / 4099 jobs with profile i % nexpect for nexpect 1, 8
  and 64, both outputs poisoned, HOST masks zero, no poison left.
* One wave that mixes operand lengths 0..64, payload lengths and depths, and
  tokens that go HOST on a number beside tokens that do not.
* No column and JG_MAX_ARGS columns of each kind.
* Every -1 of the ABI list leaves the outputs untouched; njobs == 0 returns 0.
* With ops 1..4 only the entry equals jg_claims_match.
* The older entries give the same bytes before and after a call of the new one.
"""
import ctypes
import struct

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_each_cases as EC
from tests import claims_match_args_cases as AC
from tests import claims_match_cases as MC
from tests import claims_paths_cases as PC
from tests import claims_select_cases as SC
from tests.test_gpu_claims_scan import EX, NOW, pack, sized_payload

pytestmark = pytest.mark.gpu

P = AC.P
OTHER = {"Issuer": "https://other.example/", "Audiences": ["www.example.com"]}
POISON = 0xeeeeeeee
E, W, L, H = MC.EQUALS, MC.HAS_WORD, MC.HAS_ELEMENT, MC.PRESENT
EA, GE, LE, GA, LA = AC.EQUALS_ARG, AC.NUM_GE, AC.NUM_LE, AC.NUM_GE_ARG, AC.NUM_LE_ARG
q = lambda n: struct.pack("<q", n)
# sixteen predicates on the keys the pooled payloads use: all nine ops
BATCH = AC.CORPUS_NUM + (AC.EqA(P("sub"), 1), AC.EqA(P("nonce"), 2), AC.Eq(P("nonce"), "abc"), AC.LeA(P("exp"), 3),
                         AC.Elem(P("x"), "y"), AC.Word(P("sub"), "alice@example.com"), AC.Has(P("nonce")))
assert len(BATCH) == 16 and len(AC.split(BATCH)[0]) == 8               # ... over eight paths


def enc(paths):
    return [[c.encode() if isinstance(c, str) else bytes(c) for c in p] for p in paths]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The host build of claims_match_args: the reference of the device run."""
    d = tmp_path_factory.mktemp("claims_match_args_gpu")
    AC.build_host(str(d / "claims_match_args_test"))
    return d, str(d / "claims_match_args_test")


def host_run(host, name, sets, cases, reqs, operands):
    """sets: resolved dicts; cases: (profile, segment) -> (codes, masks) of the host build"""
    d, exe = host
    path, apath = str(d / (name + ".txt")), str(d / (name + "_args.txt"))
    EC.write_sets(path, sets, cases)
    AC.write_operands(apath, operands)
    return AC.run_host(exe, path, apath, reqs)


def device_run(ctx, arena, jobs, sets, reqs, operands, lead=0):
    paths, preds = AC.split(reqs)
    args = _lib.pack_args(operands[0], operands[1], lead=lead)
    c, m = ctx.claims_match_args(arena, jobs, sets, enc(paths), preds, args)       # both outputs poisoned with 0xee
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
    jobs = [(o, l, p) for (o, l), (p, _) in zip(spans, cases)]
    codes = list(ctx.claims_each(arena, jobs, sets))
    for reqs in AC.CORPUS_SETS:
        ops = AC.derive([(seg,) for _, seg in cases], reqs)
        got = device_run(ctx, arena, jobs, sets, reqs, ops, lead=g)
        assert_host_masks_zero(got, len(reqs))
        assert_same(got, host_run(host, "corpus%d" % g, sets, cases, reqs, ops), "host build")
        if not any(op in AC.NUMERIC for _, op, _ in reqs):
            assert got[0] == codes                                      # no numeric op: no code changes
        else:
            assert all(a == b or a == _lib.CL_HOST for a, b in zip(got[0], codes))       # ... with one, only to HOST


@pytest.fixture(scope="module")
def directed_want(host):
    cases = AC.directed()
    sets = [CC.resolve({}, cases[0][2])]
    segs = [seg for seg, _, _ in cases]
    ops = AC.directed_operands()
    return {name: host_run(host, "directed", sets, [(0, s) for s in segs], reqs, ops) for name, reqs in AC.PRED_SETS.items()}


@pytest.mark.parametrize("lead", range(4))
def test_directed_list_at_every_alignment(ctx, directed_want, lead):
    cases = AC.directed()
    sets = [CC.resolve({}, cases[0][2])]
    segs = [seg for seg, _, _ in cases]
    ops = AC.directed_operands()
    arena, spans = pack(segs, lead=lead, gap=lead % 2)
    jobs = [(o, l, 0) for o, l in spans]
    for alead in range(4):
        args = _lib.pack_args(ops[0], ops[1], lead=alead)
        off, ln = args["spans"][-1][-1]
        assert ln > 0 and off + ln == len(args["bytes"])                # an operand ends at the last byte of `bytes`
        assert {o % 4 for row in args["spans"] for o, _ in row} == {0, 1, 2, 3}
        for name, reqs in AC.PRED_SETS.items():
            got = device_run(ctx, arena, jobs, sets, reqs, ops, lead=alead)
            assert_same(got, directed_want[name], (name, lead, alead))
            assert {k for k, c in enumerate(got[0]) if c == _lib.CL_HOST} == AC.directed_hosts(name)
    # the device's masks are the evaluation on the oracle's map (what the model test holds the host build to)
    for name, reqs in AC.PRED_SETS.items():
        codes, masks = directed_want[name]
        base = [_lib.CL_OK if c == _lib.CL_HOST else c for c in codes]
        AC.check(cases, base, codes, masks, reqs, ops, hosts=AC.directed_hosts(name))


def pool_segments(n):
    C = CC.corpus()
    pool = C.plain + C.hard[:200] + [(c[0], 0) for c in AC.directed()] + [(c[0], 0) for c in SC.directed()]
    return [pool[(7 * k) % len(pool)][0] for k in range(n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_batch_sizes_and_profile_counts(ctx, host, n):
    C = CC.corpus()
    all_sets = [CC.resolve(*C.sets[si]) for si in range(3, 67)]        # 64 sets with strings
    segs = pool_segments(n)
    ops = AC.derive([(s,) for s in segs], BATCH)
    arena, spans = pack(segs, lead=3)
    for nexpect in (1, 8, 64):
        sets = all_sets[:nexpect]
        jobs = [(o, l, i % nexpect) for i, (o, l) in enumerate(spans)]
        got = device_run(ctx, arena, jobs, sets, BATCH, ops, lead=1)
        assert_host_masks_zero(got, len(BATCH))
        want = host_run(host, "batch%d_%d" % (n, nexpect), sets, [(i % nexpect, s) for i, s in enumerate(segs)], BATCH, ops)
        assert_same(got, want, "nexpect %d" % nexpect)


def test_wave_mixing_operand_lengths_payloads_and_host_numbers(ctx, host):
    segs, s0, s1, n0 = [], [], [], []
    for k in range(64):
        a, b = AC.ABC[:k], AC.ABC[:64 - k]                              # lengths 0..63 and 64..1
        nonce = a if k % 3 else AC.flip(a, k // 2) if k else b"x"       # every third one differs somewhere
        auth = b"%d.5" % k if k % 7 == 3 else b"1%015d" % k if k % 7 == 5 else b"%d" % (CC.T0 - k)
        inner = b'{"jkt":"' + b + b'"}'
        for key in (b"c", b"b", b"a")[3 - k % 4:]:
            inner = b'{"' + key + b'":' + inner + b',"pad":[' + b'"p",' * (k % 5) + b"{}]}"
        filler = b'"p":"' + b"x" * (300 if k % 9 == 0 else k) + b'",'
        segs.append(CC.b64(b'{"exp":%d,"iat":%d,"iss":"https://example.com/","aud":"www.example.com",' % (CC.T0 + 600, CC.T0 - 900) + filler +
                           b'"nonce":"' + nonce + b'","auth_time":' + auth + b',"cnf":' + inner + b"}"))
        s0.append(a)
        s1.append(b)
        n0.append(CC.T0 - 32)
    segs[10] = b"e30"
    assert {len(x) for x in s0} | {len(x) for x in s1} == set(range(65))
    reqs = (AC.EqA(P("nonce"), 0), AC.GeA(P("auth_time"), 0), AC.LeA(P("auth_time"), 0), AC.EqA(P("cnf", "jkt"), 1),
            AC.EqA(P("cnf", "a", "jkt"), 1), AC.EqA(P("cnf", "a", "b", "jkt"), 1), AC.EqA(P("cnf", "a", "b", "c"), 1),
            AC.Has(P("cnf", "a", "b", "c")), AC.Ge(P("auth_time"), 0), AC.EqA(P("nonce"), 1))
    ops = ([s0, s1], [n0])
    sets = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW), CC.resolve(EX, NOW + 7200 * CC.SECOND)]
    prof = [i % 3 for i in range(64)]
    arena, spans = pack(segs, lead=1)
    jobs = [(o, l, p) for (o, l), p in zip(spans, prof)]
    got = device_run(ctx, arena, jobs, sets, reqs, ops, lead=3)
    assert_same(got, host_run(host, "wave", sets, list(zip(prof, segs)), reqs, ops))
    hosts = {k for k, c in enumerate(got[0]) if c == _lib.CL_HOST}
    assert hosts == {k for k in range(64) if k % 7 in (3, 5) and k != 10}          # the fractions and the 16 digits
    assert got[0][10] == _lib.CL_NO_TIME and {_lib.CL_OK, _lib.CL_ISS, _lib.CL_EXP} <= set(got[0])
    decided = [m for c, m in zip(*got) if c != _lib.CL_HOST]
    assert sum(m & 1 for m in decided) >= 10 and sum(1 for m in decided if not m & 1) >= 10
    assert all(any((m >> b) & 1 for m in decided) for b in (3, 4, 5, 7))           # every depth of cnf is reached
    assert any((m >> 1) & 1 for m in decided) and any((m >> 2) & 1 for m in decided)


def test_no_column_and_four_columns_of_each_kind(ctx, host):
    cases = AC.directed()
    sets = [CC.resolve({}, cases[0][2])]
    segs = [seg for seg, _, _ in cases]
    arena, spans = pack(segs, lead=2)
    jobs = [(o, l, 0) for o, l in spans]
    (a, b), (x, y) = AC.directed_operands()
    full = (AC.EqA(P("nonce"), 3), AC.EqA(P("nonce"), 0), AC.EqA(P("cnf", "jkt"), 2), AC.EqA(P("nonce"), 1),
            AC.GeA(P("auth_time"), 3), AC.LeA(P("auth_time"), 0), AC.GeA(P("auth_time"), 2), AC.LeA(P("auth_time"), 1),
            AC.Ge(P("auth_time"), 0), AC.Has(P("nonce")))
    for ops, reqs in ((([], []), MC.SCOPE), (([], []), (AC.Ge(P("auth_time"), 0), AC.Le(P("exp"), CC.T0 + 5))),
                      (([a, b, a, b], [x, y, y, x]), full), (([b, a, b, a], []), full[:4] + full[8:]),
                      (([], [x, y, y, x]), full[4:])):
        got = device_run(ctx, arena, jobs, sets, reqs, ops, lead=1)
        assert_same(got, host_run(host, "cols", sets, [(0, s) for s in segs], reqs, ops), (len(ops[0]), len(ops[1])))
        assert any(got[1])


def test_old_ops_equal_claims_match(ctx):
    segs = pool_segments(300)
    arena, spans = pack(segs, lead=1)
    sets = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW)]
    jobs = [(o, l, i % 2) for i, (o, l) in enumerate(spans)]
    ops = AC.derive([(s,) for s in segs], MC.FULL, nstr=2, nnum=1)
    for reqs in (MC.FULL, MC.SCOPE, MC.CORPUS_SETS[1], ()):
        paths, preds = MC.split(reqs)
        c, m = ctx.claims_match(arena, jobs, sets, enc(paths), preds)
        assert device_run(ctx, arena, jobs, sets, reqs, ([], [])) == (list(c), m)
        assert device_run(ctx, arena, jobs, sets, reqs, ops, lead=2) == (list(c), m)      # idle columns change nothing
    assert len(set(c)) >= 4


def raw_call(ctx, preds, args, null=(), jobs=((0, 3, 0),), nexpect=1, paths=((b"a", b"b"), (b"c",)), arena=b"e30"):
    """One call with poisoned outputs -> (rc, codes + masks as bytes)"""
    n = len(jobs)
    e = _lib.JgExpect()
    e.now_sec = CC.T0
    ps, _k1 = _lib._jg_paths(paths)
    qs, _k2 = _lib._jg_preds(preds)
    ga, _k3 = _lib._jg_args(args, null)
    out = ctypes.create_string_buffer(b"\xee" * n, n)
    m = ctypes.create_string_buffer(b"\xee" * 4 * n, 4 * n)
    rc = _lib.lib().jg_claims_match_args(ctx.h, arena, len(arena), _lib._cjobs(jobs), n, ctypes.byref(e), nexpect,
                                         ctypes.byref(ps), ctypes.byref(qs), None if "args" in null else ctypes.byref(ga),
                                         out, ctypes.cast(m, ctypes.c_void_p))
    return rc, out.raw + m.raw


def test_bad_arguments_and_empty_batch(ctx):
    ex = CC.resolve(EX, NOW)
    untouched = (-1, b"\xee" * 5)
    two = _lib.pack_args([[b"x"], [b"yy"]], [[1], [2]])
    ok = [(0, EA, b"\0"), (1, GA, b"\x01"), (1, GE, q(5))]
    assert raw_call(ctx, ok, two) == (0, bytes([_lib.CL_NO_TIME]) + bytes(4))
    # the column counts, a column index past its count, a wrong value_len
    assert raw_call(ctx, [], _lib.pack_args([[b"x"]] * 5, [])) == untouched
    assert raw_call(ctx, [], _lib.pack_args([], [[1]] * 5)) == untouched
    assert "jg_claims_match_args" in ctx.error() and "columns" in ctx.error()
    for preds in ([(0, EA, b"\x02")], [(0, GA, b"\x02")], [(1, LA, b"\xff")], [(0, EA, b"")], [(0, EA, b"\0\0")],
                  [(0, GA, b"")], [(0, LA, b"\0\0")], [(0, GE, b"")], [(0, GE, q(1)[:7])], [(0, LE, q(1) + b"\0")],
                  # the same path, op and column
                  [(0, EA, b"\0"), (1, EA, b"\0"), (0, EA, b"\0")], [(1, GA, b"\x01"), (1, GA, b"\x01")],
                  [(0, GE, q(5)), (0, GE, q(5))],
                  # everything jg_claims_match refuses
                  [(0, 0, b"x")], [(0, 10, b"\0")], [(0, 255, b"x")], [(2, E, b"x")], [(0, W, b"a b")], [(0, H, b"x")],
                  [(0, E, b"v" * 65)], [(0, L, b"")], [(0, E, b"a\x80")], [(0, E, b"x"), (0, E, b"x")],
                  [(k % 2, GE, q(k)) for k in range(17)]):
        assert raw_call(ctx, preds, two) == untouched, preds
    assert raw_call(ctx, [(0, EA, b"\0")], _lib.pack_args([], [[1]])) == untouched       # no string column at all
    assert raw_call(ctx, ok, two, jobs=[(0, 3, 1)]) == untouched
    assert raw_call(ctx, ok, two, jobs=[(1, 3, 0)]) == untouched
    assert raw_call(ctx, ok, two, nexpect=65) == untouched
    assert raw_call(ctx, ok, two, paths=[[]]) == untouched
    assert raw_call(ctx, ok, two, paths=[[b"a"], [b"a"]]) == untouched
    # args, or a needed array of it, NULL
    for null in ("args", "bytes", "str", "num"):
        assert raw_call(ctx, ok, two, null=(null,)) == untouched, null
    assert raw_call(ctx, [(0, GE, q(1))], _lib.pack_args([], []), null=("bytes", "str", "num")) == \
        (0, bytes([_lib.CL_NO_TIME]) + bytes(4))                         # ... but not where nothing is needed
    # operands: a refused byte, a len over JG_PRED_VALUE_MAX, a span past bytes_len, each naming the job
    three = [(0, 3, 0)] * 3
    for v in (b"a\x1fb", b"a\x7f", b"\x80", b'a"b', b"a\\b", b"a\0b", b"v" * 65):
        rc, out = raw_call(ctx, ok, _lib.pack_args([[b"x", b"x", v], [b"y"] * 3], [[1] * 3, [2] * 3]), jobs=three)
        assert (rc, out) == (-1, b"\xee" * 15) and "job 2" in ctx.error(), v
    for span in ((4, 1), (0, 5), (3, 2), (0xffffffff, 2), (1, 0xffffffff), (5, 0)):
        a = _lib.pack_args([[b"x", b"ab", b"c"], [b"", b"", b""]], [[1] * 3, [2] * 3])
        assert len(a["bytes"]) == 4
        a["spans"][1][1] = span
        rc, out = raw_call(ctx, ok, a, jobs=three)
        assert (rc, out) == (-1, b"\xee" * 15) and "job 1" in ctx.error(), span
    a = _lib.pack_args([[b"x", b"ab", b"c"], [b"", b"", b""]], [[1] * 3, [2] * 3])
    a["spans"][1][1] = (4, 0)                                            # an empty span at the very end is inside
    assert raw_call(ctx, ok, a, jobs=three)[0] == 0
    # njobs == 0 returns 0 whatever else is NULL
    assert raw_call(ctx, ok, two, jobs=[], null=("args",)) == (0, b"")
    assert ctx.claims_match_args(b"", [], [ex], [[b"a"]], [(0, EA, b"\0")], _lib.pack_args([[]], []),
                                 null=("paths", "preds", "args", "codes", "masks")) == (b"", [])
    # jg_claims_match keeps refusing the new ops
    for op in (5, 6, 7, 8, 9, 255):
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.claims_match(b"e30", [(0, 3, 0)], [ex], [[b"a"]], [(0, op, b"\0")])
    # then a good call on the same context
    seg = CC.b64(b'{"nonce":"n-1","auth_time":%d,"exp":%d}' % (CC.T0, CC.T0 + 600))
    codes, masks = ctx.claims_match_args(seg, [(0, len(seg), 1)], [CC.resolve({}, NOW), ex], [[b"nonce"], [b"auth_time"]],
                                         [(0, EA, b"\0"), (1, GA, b"\0"), (1, LA, b"\0"), (0, EA, b"\x01"), (1, LE, q(CC.T0))],
                                         _lib.pack_args([[b"n-1"], [b"n-2"]], [[CC.T0 - 1]]))
    assert codes == bytes([_lib.CL_ISS]) and masks == [0b10011]


def test_old_entries_unchanged_around_a_call(ctx):
    segs = pool_segments(300)
    arena, spans = pack(segs, lead=2)
    sets = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW)]
    jobs = [(o, l, i % 2) for i, (o, l) in enumerate(spans)]
    names = [n.encode() for n in SC.EIGHT]
    paths, preds = MC.split(MC.FULL)

    def old():
        a = ctx.claims_each(arena, jobs, sets, mode="select", names=names)
        b = ctx.claims_paths(arena, jobs, sets, enc(PC.EIGHT))
        return (a[0], bytes(a[1]), bytes(a[2]), b[0], bytes(b[1]), bytes(b[2]), ctx.claims_match(arena, jobs, sets, enc(paths), preds),
                ctx.claims_scan(arena, spans, sets[1]), bytes(ctx.claims_extract(arena, spans, sets[0])[1]))
    before = old()
    ops = AC.derive([(s,) for s in segs[:70]], BATCH)
    small = device_run(ctx, arena, jobs[:70], sets, BATCH, ops)           # a smaller batch: the kept buffers are shared
    assert old() == before
    assert device_run(ctx, arena, jobs[:70], sets, BATCH, ops) == small
    assert len(set(before[0])) >= 5 and any(small[1])
