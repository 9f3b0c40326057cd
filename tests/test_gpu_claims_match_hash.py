"""k_hash_operand + k_claims_match_args through the C ABI (jg_claims_match_hash /
Context.claims_match_hash).

(a) For jobs with a family, EQUALS_HASH(h) gives the codes and masks of
    jg_claims_match_args with EQUALS_ARG on a string column that holds the hashlib
    value, byte for byte: a pool of corpus payloads and payloads that carry
    at_hash / c_hash, 1 / 63 / 64 / 65 / 257 / 4099 jobs, nexpect 1, 8 and 64, both
    outputs poisoned, HOST masks zero; a quarter of the sources differ from the
    truth in their first or last byte.
(b) IS_STRING (and everything else) against the host build of the same code
    (tests/host_unit/claims_match_hash_test.cpp): the directed list at several
    alignments, a corpus group.
(c) One wave that mixes the three families, family 0, source lengths 0..8192,
    plain string and number columns beside the hashed ones and tokens that go
    HOST on a fraction, in the shapes 2+2 and 3+1.
(d) Every -1 of the ABI list leaves both outputs untouched; njobs == 0; a good
    call follows on the same context.
(e) With no op >= 10 and nhash 0 the entry equals jg_claims_match_args.
(f) The older entries give the same bytes before and after a call.
"""
import ctypes

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_each_cases as EC
from tests import claims_match_args_cases as AC
from tests import claims_match_cases as MC
from tests import claims_match_hash_cases as HC
from tests import claims_paths_cases as PC
from tests import claims_select_cases as SC
from tests.test_gpu_claims_match_args import BATCH, OTHER, assert_host_masks_zero, assert_same, enc, pool_segments, q
from tests.test_gpu_claims_scan import EX, NOW, pack

pytestmark = pytest.mark.gpu

P = HC.P
E, H = MC.EQUALS, MC.PRESENT
EA, GE, GA, EH, IS = AC.EQUALS_ARG, AC.NUM_GE, AC.NUM_GE_ARG, HC.EQUALS_HASH, HC.IS_STRING


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The host build of the scan and of hash_operand: the reference of the device run."""
    d = tmp_path_factory.mktemp("claims_match_hash_gpu")
    HC.build_host(str(d / "claims_match_hash_test"))
    return d, str(d / "claims_match_hash_test")


def host_run(host, name, sets, cases, reqs, operands):
    d, exe = host
    path, apath = str(d / (name + ".txt")), str(d / (name + "_args.txt"))
    EC.write_sets(path, sets, cases)
    HC.write_operands(apath, operands)
    return HC.run_host(exe, path, apath, reqs)


def device_run(ctx, arena, jobs, sets, reqs, operands, lead=0, hlead=0):
    paths, preds = HC.split(reqs)
    strs, nums, hashes = operands
    args = _lib.pack_args(strs, nums, lead=lead)
    hargs = _lib.pack_hargs(hashes, lead=hlead)
    c, m = ctx.claims_match_hash(arena, jobs, sets, enc(paths), preds, args, hargs)    # both outputs poisoned with 0xee
    assert len(c) == len(jobs) == len(m)
    return list(c), m


def args_run(ctx, arena, jobs, sets, reqs, strs, nums, lead=0):
    paths, preds = AC.split(reqs)
    c, m = ctx.claims_match_args(arena, jobs, sets, enc(paths), preds, _lib.pack_args(strs, nums, lead=lead))
    return list(c), m


# ---- (a) ----
# the hashed form and its twin for jg_claims_match_args: string column 0 is the nonce, 1 and 2 hold the hashlib values
HASHED = (HC.EqH(P("at_hash"), 0), AC.EqA(P("nonce"), 0), HC.EqH(P("c_hash"), 1), MC.Has(P("at_hash")),
          HC.EqH(P("sub"), 0), AC.Ge(P("exp"), CC.T0), MC.Elem(P("aud"), "www.example.com"), HC.EqH(P("at_hash"), 1),
          AC.GeA(P("iat"), 0))
TWIN = (AC.EqA(P("at_hash"), 1), AC.EqA(P("nonce"), 0), AC.EqA(P("c_hash"), 2), MC.Has(P("at_hash")),
        AC.EqA(P("sub"), 1), AC.Ge(P("exp"), CC.T0), MC.Elem(P("aud"), "www.example.com"), AC.EqA(P("at_hash"), 2),
        AC.GeA(P("iat"), 0))


def hash_pool(n):
    """n payload segments, every other one with at_hash / c_hash for its own token and code, and per job the nonce,
    the truth (token, code, family) and the sources the call is given: a quarter differ in their first or last byte"""
    corpus = pool_segments(n)
    segs, nonce, truth, given = [], [], [], []
    for k in range(n):
        fam = HC.FAMS[k % 3]
        tok, code = HC.source(k, 40 if k % 5 else (k % 97)), HC.source(k + 100000, 22 + k % 9)
        if k % 2 == 0:
            claims = {"iss": "https://example.com/", "aud": ["www.example.com"] if k % 3 else "www.example.com", "sub": "alice@example.com",
                      "exp": CC.T0 + (600 if k % 7 else -600), "iat": CC.T0 - k % 50, "nonce": "n-%d" % k,
                      "at_hash": HC.hash_value(tok, fam).decode(), "c_hash": HC.hash_value(code, fam).decode()}
            if k % 10 == 4:
                claims["sub"] = claims["at_hash"]                               # EQUALS_HASH(sub, 0) holds somewhere
            segs.append(CC.b64(CC.js(claims)))
        else:
            segs.append(corpus[k])
        nonce.append(b"n-%d" % (k if k % 6 else k + 1))
        truth.append((tok, code, fam))
        wrong = (k >> 1) % 4 == 1
        flip = lambda v, at: v if not (wrong and v) else AC.flip(v, at)
        given.append((flip(tok, 0 if k % 3 else len(tok) - 1), flip(code, len(code) - 1 if k % 3 else 0), fam))
    return segs, nonce, truth, given


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_equals_hash_is_equals_arg_on_the_hashlib_value(ctx, n):
    C = CC.corpus()
    all_sets = [CC.resolve(*C.sets[si]) for si in range(3, 67)]
    segs, nonce, truth, given = hash_pool(n)
    arena, spans = pack(segs, lead=3)
    hashes = [[(t, fam) for t, _, fam in given], [(c, fam) for _, c, fam in given]]
    values = [[HC.hash_value(t, fam) for t, _, fam in given], [HC.hash_value(c, fam) for _, c, fam in given]]
    nums = [[CC.T0 - 25] * n]
    assert abs(4 * sum(1 for g, t in zip(given, truth) if g != t) - n) <= 16     # a quarter of the sources are wrong
    for nexpect in (1, 8, 64):
        sets = [CC.resolve(EX, NOW)] + all_sets[:nexpect - 1]
        jobs = [(o, l, i % nexpect) for i, (o, l) in enumerate(spans)]
        got = device_run(ctx, arena, jobs, sets, HASHED, ([nonce], nums, hashes), lead=1, hlead=nexpect % 4)
        assert_host_masks_zero(got, len(HASHED))
        want = args_run(ctx, arena, jobs, sets, TWIN, [nonce] + values, nums, lead=2)
        assert_same(got, want, "nexpect %d" % nexpect)
        if n >= 257:
            decided = [m for c, m in zip(*got) if c != _lib.CL_HOST]
            for bit in (0, 2):                                                   # at_hash and c_hash against their columns
                hits = sum((m >> bit) & 1 for m in decided)
                assert hits >= 25 and len(decided) - hits >= 100, (bit, hits, len(decided))
            assert any((m >> 4) & 1 for m in decided) and not any((m >> 7) & 1 for m in decided)
            # ... and the hits are the payloads whose own token was given
            for k, (c, m) in enumerate(zip(*got)):
                if k % 2 == 0 and c != _lib.CL_HOST:
                    assert m & 1 == (given[k][0] == truth[k][0]) and (m >> 2) & 1 == (given[k][1] == truth[k][1]), k


# ---- (b) ----
@pytest.mark.parametrize("lead", range(4))
def test_directed_list_equals_host_build(ctx, host, lead):
    cases = HC.directed()
    sets = [CC.resolve({}, cases[0][2])]
    segs = [seg for seg, _, _ in cases]
    ops = HC.directed_operands()
    arena, spans = pack(segs, lead=lead, gap=lead % 2)
    jobs = [(o, l, 0) for o, l in spans]
    h = _lib.pack_hargs(ops[2], lead=lead)
    assert h["src"][-1][-1][1] > 0 and sum(h["src"][-1][-1][:2]) == len(h["bytes"])     # a source ends at the last byte
    for name, reqs in HC.PRED_SETS.items():
        want = host_run(host, "directed", sets, [(0, s) for s in segs], reqs, ops)
        got = device_run(ctx, arena, jobs, sets, reqs, ops, lead=(lead + 1) % 4, hlead=lead)
        assert_same(got, want, (name, lead))
        assert _lib.CL_HOST not in got[0]
        if lead == 0:                                                            # ... which is the evaluation on the oracle's map
            HC.check(cases, got[0], got[0], got[1], reqs, ops)


def test_corpus_group_equals_host_build(ctx, host):
    C = CC.corpus()
    lo, hi = EC.groups()[1]
    allc = C.all_cases()
    idx = EC.group_cases(lo, hi)
    sets = [CC.resolve(*C.sets[si]) for si in range(lo, hi)]
    cases = [(allc[k][1] - lo, allc[k][0]) for k in idx]
    arena, spans = pack([seg for _, seg in cases], lead=2, gap=1)
    jobs = [(o, l, p) for (o, l), (p, _) in zip(spans, cases)]
    codes = list(ctx.claims_each(arena, jobs, sets))
    for reqs in HC.CORPUS_SETS:
        ops = HC.derive([(seg,) for _, seg in cases], reqs)
        got = device_run(ctx, arena, jobs, sets, reqs, ops, lead=1, hlead=3)
        assert_host_masks_zero(got, len(reqs))
        assert_same(got, host_run(host, "corpus", sets, cases, reqs, ops), "host build")
        assert all(a == b or a == _lib.CL_HOST for a, b in zip(got[0], codes))   # only the numeric op's rule changes a code
        # the new ops alone change none
        only = tuple(r for r in reqs if r[1] >= HC.EQUALS_HASH or r[1] <= MC.PRESENT)
        assert device_run(ctx, arena, jobs, sets, only, ops, hlead=1)[0] == codes


# ---- (c) ----
@pytest.mark.parametrize("shape", [(2, 2), (3, 1)])
def test_wave_mixing_families_lengths_columns_and_host_numbers(ctx, host, shape):
    nstr, nhash = shape
    lens = list(range(0, 40)) + [54, 55, 56, 63, 64, 65, 111, 112, 119, 120, 127, 128, 129, 239, 240, 1000, 4096, 8191, 8192,
                                 8192, 300, 77, 5, 0]
    assert len(lens) == 64
    segs, strs, hashes, n0 = [], [[] for _ in range(nstr)], [[] for _ in range(nhash)], []
    for k in range(64):
        fam = (k % 4)                                                            # 0: no value
        tok, code = HC.source(k, lens[k]), HC.source(k + 500, lens[63 - k])
        right = HC.hash_value(tok, fam or 1)
        at = right if k % 3 else AC.flip(right, k % len(right))
        ch = HC.hash_value(code, fam or 2)
        auth = b"%d.5" % k if k % 7 == 3 else b"%d" % (CC.T0 - k)
        at_member = (b'"at_hash":"' + at + b'"', b'"at_hash":%d' % k, b'"at_hash":""', b'"at_hash":null')[0 if k % 8 else (k // 8) % 4]
        filler = b'"p":"' + b"x" * (300 if k % 9 == 0 else k) + b'",'
        segs.append(CC.b64(b'{"exp":%d,"iat":%d,"iss":"https://example.com/","aud":"www.example.com",' % (CC.T0 + 600, CC.T0 - 900) +
                           filler + b'"nonce":"n-%d",' % k + at_member + b',"auth_time":' + auth +
                           b',"oidc":{"c_hash":"' + ch + b'"}}'))
        for c in range(nstr):
            strs[c].append((b"n-%d" % (k + (k % 5 == 0)), AC.ABC[:k], at)[c])
        hashes[0].append((tok, fam) if fam else None)
        if nhash > 1:
            hashes[1].append((code, fam) if fam else None)
        n0.append(CC.T0 - 32)
    segs[10] = b"e30"
    reqs = (HC.EqH(P("at_hash"), 0), HC.IsStr(P("at_hash")), AC.EqA(P("nonce"), 0), AC.GeA(P("auth_time"), 0),
            HC.EqH(P("oidc", "c_hash"), nhash - 1), HC.IsStr(P("oidc", "c_hash")), HC.IsStr(P("oidc")), AC.EqA(P("nonce"), 1),
            AC.EqA(P("at_hash"), nstr - 1), MC.Has(P("at_hash")), HC.IsStr(P("auth_time")))
    ops = (strs, [n0], hashes)
    sets = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW), CC.resolve(EX, NOW + 7200 * CC.SECOND)]
    prof = [i % 3 for i in range(64)]
    arena, spans = pack(segs, lead=1)
    jobs = [(o, l, p) for (o, l), p in zip(spans, prof)]
    got = device_run(ctx, arena, jobs, sets, reqs, ops, lead=3, hlead=2)
    assert_same(got, host_run(host, "wave%d" % nstr, sets, list(zip(prof, segs)), reqs, ops))
    assert {k for k, c in enumerate(got[0]) if c == _lib.CL_HOST} == {k for k in range(64) if k % 7 == 3 and k != 10}
    assert got[0][10] == _lib.CL_NO_TIME and {_lib.CL_OK, _lib.CL_ISS, _lib.CL_EXP} <= set(got[0])
    decided = {k: m for k, (c, m) in enumerate(zip(*got)) if c != _lib.CL_HOST and k != 10}
    for k, m in decided.items():
        is_str = k % 8 != 0 or (k // 8) % 4 in (0, 2)                            # 0: the value, 2: ""
        assert (m >> 1) & 1 == is_str and (m >> 9) & 1 == 1 and (m >> 10) & 1 == 0 and (m >> 6) & 1 == 0, k
        assert m & 1 == (k % 4 != 0 and k % 3 != 0), k                          # a family and the right value (then it is a string)
        same_src = lens[k] == 0 and lens[63 - k] == 0                            # one hash column: c_hash against the token's hash
        assert (m >> 5) & 1 == 1 and (m >> 4) & 1 == (k % 4 != 0 and (nhash == 2 or same_src)), k
    assert sum(m & 1 for m in decided.values()) >= 10
    if nstr == 3:                                                                # the plain column that holds at_hash's own text
        assert all((m >> 8) & 1 == (k % 8 != 0 or (k // 8) % 4 == 0) for k, m in decided.items())


# ---- (d) ----
def raw_call(ctx, preds, args, hargs, null=(), jobs=((0, 3, 0),), nexpect=1, paths=((b"a", b"b"), (b"c",)), arena=b"e30"):
    """One call with poisoned outputs -> (rc, codes + masks as bytes)"""
    n = len(jobs)
    e = _lib.JgExpect()
    e.now_sec = CC.T0
    ps, _k1 = _lib._jg_paths(paths)
    qs, _k2 = _lib._jg_preds(preds)
    ga, _k3 = _lib._jg_args(args, null) if args is not None else (None, None)
    gh, _k4 = _lib._jg_hargs(hargs, null) if hargs is not None else (None, None)
    out = ctypes.create_string_buffer(b"\xee" * n, n)
    m = ctypes.create_string_buffer(b"\xee" * 4 * n, 4 * n)
    rc = _lib.lib().jg_claims_match_hash(ctx.h, arena, len(arena), _lib._cjobs(jobs), n, ctypes.byref(e), nexpect,
                                         ctypes.byref(ps), ctypes.byref(qs), None if ga is None else ctypes.byref(ga),
                                         None if gh is None else ctypes.byref(gh), out, ctypes.cast(m, ctypes.c_void_p))
    return rc, out.raw + m.raw


def test_bad_arguments_and_empty_batch(ctx):
    ex = CC.resolve(EX, NOW)
    untouched = (-1, b"\xee" * 5)
    good = (0, bytes([_lib.CL_NO_TIME]) + bytes(4))
    two = _lib.pack_args([[b"x"], [b"yy"]], [[1], [2]])
    h2 = _lib.pack_hargs([[(b"tok", 1)], [None]])
    ok = [(0, EA, b"\0"), (1, GA, b"\x01"), (1, GE, q(5)), (0, EH, b"\x01"), (1, IS, b""), (0, EH, b"\0")]
    assert raw_call(ctx, ok, two, h2) == good
    assert raw_call(ctx, [(0, EH, b"\0"), (0, IS, b"")], None, h2) == good                    # args NULL: no plain columns
    assert raw_call(ctx, [(0, IS, b""), (0, EA, b"\0")], two, None) == good                   # hargs NULL: nhash 0
    assert raw_call(ctx, [(0, IS, b"")], None, None) == good
    # the column counts
    three = _lib.pack_hargs([[(b"t", 1)]] * 3)
    assert raw_call(ctx, [], None, three) == untouched
    assert "jg_claims_match_hash" in ctx.error() and "hash columns" in ctx.error()
    assert raw_call(ctx, [], _lib.pack_args([[b"x"]] * 3, []), h2) == untouched
    assert raw_call(ctx, [], _lib.pack_args([[b"x"]] * 4, []), _lib.pack_hargs([[(b"t", 1)]])) == untouched
    assert raw_call(ctx, [], _lib.pack_args([[b"x"]] * 5, []), None) == untouched
    assert raw_call(ctx, [(1, EH, b"\0")], _lib.pack_args([[b"x"]] * 3, []), _lib.pack_hargs([[(b"t", 1)]])) == good
    for preds in ([(0, EH, b"\x02")], [(0, EH, b"\xff")], [(0, EH, b"")], [(0, EH, b"\0\0")], [(0, IS, b"x")],
                  # two EQUALS_HASH on the same path and column, two IS_STRING on one path
                  [(0, EH, b"\0"), (1, EH, b"\0"), (0, EH, b"\0")], [(1, IS, b""), (0, IS, b""), (1, IS, b"")],
                  # the ops outside 1..11, and everything jg_claims_match_args refuses
                  [(0, 0, b"x")], [(0, 12, b"")], [(0, 255, b"x")], [(2, IS, b"")], [(0, EA, b"\x02")], [(0, GE, b"")],
                  [(0, E, b"a\x80")], [(0, EA, b"\0"), (0, EA, b"\0")], [(k % 2, GE, q(k)) for k in range(17)]):
        assert raw_call(ctx, preds, two, h2) == untouched, preds
        assert "jg_claims_match_hash" in ctx.error()
    assert raw_call(ctx, [(0, EH, b"\0")], two, None) == untouched                           # no hash column at all
    assert raw_call(ctx, ok, two, h2, jobs=[(0, 3, 1)]) == untouched
    assert raw_call(ctx, ok, two, h2, jobs=[(1, 3, 0)]) == untouched
    assert raw_call(ctx, ok, two, h2, nexpect=65) == untouched
    assert raw_call(ctx, ok, two, h2, paths=[[b"a"], [b"a"]]) == untouched
    # a needed array NULL
    for null in ("bytes", "str", "num", "hbytes", "hsrc"):
        assert raw_call(ctx, ok, two, h2, null=(null,)) == untouched, null
    assert raw_call(ctx, [(0, EH, b"\0")], None, _lib.pack_hargs([[(b"", 3)]]), null=("hbytes",)) == good    # ... but not where nothing is needed
    big = dict(h2, bytes_len=1 << 32)
    assert raw_call(ctx, ok, two, big) == untouched
    # sources: a len over JG_HASH_SRC_MAX, a span past bytes_len, a fam outside 0..3, each naming the job
    jobs3 = [(0, 3, 0)] * 3
    a3 = _lib.pack_args([[b"x"] * 3, [b"y"] * 3], [[1] * 3, [2] * 3])
    for src in ((0, 8193, 1), (0, 1, 4), (0, 1, 255), (9000, 1, 1), (8999, 2, 1), (0xffffffff, 2, 1), (1, 0xffffffff, 2)):
        h = _lib.pack_hargs([[(b"t" * 3000, 1)] * 3, [(b"", 2)] * 3])
        assert len(h["bytes"]) == 9000
        h["src"][1][1] = src
        rc, out = raw_call(ctx, ok, a3, h, jobs=jobs3)
        assert (rc, out) == (-1, b"\xee" * 15) and "job 1" in ctx.error() and "jg_claims_match_hash" in ctx.error(), src
    h = _lib.pack_hargs([[(b"t" * 3000, 1)] * 3, [(b"", 2)] * 3])
    h["src"][1][1] = (9000, 0, 0)                                                # an empty span at the very end is inside
    h["src"][2][0] = (808, 8192, 3)                                              # ... and so is the longest source, up to the last byte
    assert raw_call(ctx, ok, a3, h, jobs=jobs3)[0] == 0
    # a refused plain operand still names its job
    rc, out = raw_call(ctx, ok, _lib.pack_args([[b"x", b"x", b"a\x1fb"], [b"y"] * 3], [[1] * 3, [2] * 3]), h, jobs=jobs3)
    assert (rc, out) == (-1, b"\xee" * 15) and "job 2" in ctx.error()
    # njobs == 0 returns 0 whatever else is NULL
    assert raw_call(ctx, ok, None, None, jobs=[]) == (0, b"")
    assert ctx.claims_match_hash(b"", [], [ex], [[b"a"]], [(0, EH, b"\0")], None, None,
                                 null=("paths", "preds", "codes", "masks")) == (b"", [])
    # the older entries keep refusing the new ops
    for op in (10, 11):
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.claims_match(b"e30", [(0, 3, 0)], [ex], [[b"a"]], [(0, op, b"\0")])
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.claims_match_args(b"e30", [(0, 3, 0)], [ex], [[b"a"]], [(0, op, b"\0" if op == 10 else b"")], two)
    # then a good call on the same context
    tok = b"SlAV32hkKG"
    seg = CC.b64(b'{"nonce":"n-1","at_hash":"%s","exp":%d}' % (HC.hash_value(tok, 1), CC.T0 + 600))
    codes, masks = ctx.claims_match_hash(seg, [(0, len(seg), 1)], [CC.resolve({}, NOW), ex], [[b"nonce"], [b"at_hash"]],
                                         [(0, EA, b"\0"), (1, EH, b"\0"), (1, IS, b""), (1, EH, b"\x01"), (0, IS, b"")],
                                         _lib.pack_args([[b"n-1"]], []), _lib.pack_hargs([[(tok, 1)], [(tok, 2)]]))
    assert codes == bytes([_lib.CL_ISS]) and masks == [0b10111]


# ---- (e) ----
def test_without_new_ops_equals_claims_match_args(ctx):
    segs = pool_segments(300)
    arena, spans = pack(segs, lead=1)
    sets = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW)]
    jobs = [(o, l, i % 2) for i, (o, l) in enumerate(spans)]
    strs, nums = AC.derive([(s,) for s in segs], BATCH)
    want = args_run(ctx, arena, jobs, sets, BATCH, strs, nums, lead=2)
    paths, preds = AC.split(BATCH)
    args = _lib.pack_args(strs, nums, lead=2)
    for hargs in (None, _lib.pack_hargs([]), dict(_lib.pack_hargs([]), bytes=b"unused")):
        c, m = ctx.claims_match_hash(arena, jobs, sets, enc(paths), preds, args, hargs)
        assert (list(c), m) == want
    assert len(set(want[0])) >= 4 and any(want[1])
    # idle hash columns change nothing either (two string columns leave room for two)
    reqs = AC.NONCE
    s2 = AC.derive([(s,) for s in segs], reqs, nstr=2, nnum=0)[0]
    idle = [[(HC.source(k, k % 90), 1 + k % 3) for k in range(300)], [None] * 300]
    assert device_run(ctx, arena, jobs, sets, reqs, (s2, [], idle)) == args_run(ctx, arena, jobs, sets, reqs, s2, [])


# ---- (f) ----
def test_old_entries_unchanged_around_a_call(ctx):
    segs, nonce, _, given = hash_pool(300)
    arena, spans = pack(segs, lead=2)
    sets = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW)]
    jobs = [(o, l, i % 2) for i, (o, l) in enumerate(spans)]
    names = [n.encode() for n in SC.EIGHT]
    paths, preds = MC.split(MC.FULL)
    astrs, anums = AC.derive([(s,) for s in segs], BATCH)

    def old():
        a = ctx.claims_each(arena, jobs, sets, mode="select", names=names)
        b = ctx.claims_paths(arena, jobs, sets, enc(PC.EIGHT))
        return (a[0], bytes(a[1]), bytes(a[2]), b[0], bytes(b[1]), bytes(b[2]), ctx.claims_match(arena, jobs, sets, enc(paths), preds),
                args_run(ctx, arena, jobs, sets, BATCH, astrs, anums), ctx.claims_scan(arena, spans, sets[1]),
                bytes(ctx.claims_extract(arena, spans, sets[0])[1]))
    before = old()
    ops = ([nonce[:70]], [[CC.T0] * 70], [[(t, f) for t, _, f in given[:70]], [(c, f) for _, c, f in given[:70]]])
    small = device_run(ctx, arena, jobs[:70], sets, HASHED, ops)                 # a smaller batch: the kept buffers are shared
    assert old() == before
    assert device_run(ctx, arena, jobs[:70], sets, HASHED, ops) == small
    assert len(set(before[0])) >= 4 and any(m & 1 for m in small[1])
