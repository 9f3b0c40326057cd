"""k_claims_match_set through the C ABI (jg_set_load + jg_claims_match_set /
Context.claims_match_set).

(a) The twin test: IN_SET against a k-member set is the OR of k EQUALS bits of
    jg_claims_match, ELEMENT_IN_SET the OR of k HAS_ELEMENT bits, codes and all:
    k = 1, 2 and 16, 1 / 63 / 64 / 65 / 257 / 4099 jobs, nexpect 1, 8 and 64, both
    outputs poisoned, HOST masks zero.
(b) Codes and masks against the host build of the same code
    (tests/host_unit/claims_match_set_test.cpp): the directed list and every
    group of the corpus, each at arena offsets 0..3 mod 4.
(c) One wave that mixes hits, misses, a miss of a member's hash, 0- and 255-byte
    values, HOST tokens, segments of 3 and of some 400 characters and arrays of
    0..40 elements.
(d) Every -1 of the ABI list leaves both outputs untouched; njobs == 0; a good
    call follows on the same context.
(e) With no op >= 12 the entry equals jg_claims_match_hash.
(f) The older entries give the same bytes before and after a call.
(g) A jg_set_load that replaces an id between two scans changes the second
    scan's masks and nothing else.
"""
import ctypes

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_each_cases as EC
from tests import claims_match_args_cases as AC
from tests import claims_match_cases as MC
from tests import claims_match_hash_cases as HC
from tests import claims_match_set_cases as TC
from tests import claims_paths_cases as PC
from tests import claims_select_cases as SC
from tests import set_model as SM
from tests.claims_match_set_cases import BATCH, OTHER, assert_host_masks_zero, assert_same, enc, pool_segments
from tests.test_gpu_claims_scan import EX, NOW, pack

pytestmark = pytest.mark.gpu

P = TC.P
E, L, H = MC.EQUALS, MC.HAS_ELEMENT, MC.PRESENT
EA, GE, EH, IS, IN, EL = AC.EQUALS_ARG, AC.NUM_GE, HC.EQUALS_HASH, HC.IS_STRING, TC.IN_SET, TC.ELEMENT_IN_SET


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The host build of the scan and of set_build: the reference of the device run."""
    d = tmp_path_factory.mktemp("claims_match_set_gpu")
    TC.build_host(str(d / "claims_match_set_test"))
    return d, str(d / "claims_match_set_test")


def host_run(host, name, profs, cases, reqs, operands, call_sets):
    d, exe = host
    path, apath, spath = str(d / (name + ".txt")), str(d / (name + "_args.txt")), str(d / (name + "_sets.txt"))
    EC.write_sets(path, profs, cases)
    HC.write_operands(apath, operands)
    TC.write_sets(spath, call_sets)
    return TC.run_host(exe, path, apath, spath, reqs)


def load(ctx, call_sets, first=0):
    """Loads the call's sets as ids first.. -> the ids"""
    ids = list(range(first, first + len(call_sets)))
    for i, (members, seed) in zip(ids, call_sets):
        ctx.set_load(i, members, seed)
    return ids


def device_run(ctx, arena, jobs, profs, reqs, operands, ids, lead=0):
    paths, preds = TC.split(reqs)
    strs, nums, hashes = operands
    args = _lib.pack_args(strs, nums, lead=lead) if strs or nums else None
    hargs = _lib.pack_hargs(hashes) if hashes else None
    c, m = ctx.claims_match_set(arena, jobs, profs, enc(paths), preds, args, hargs, ids)    # both outputs poisoned with 0xee
    assert len(c) == len(jobs) == len(m)
    return list(c), m


# ---- (a) ----
def set_pool(n):
    """n payload segments: the pool of the older tests and, every other one, a payload with one of 37 subjects and
    an audience that is a string or an array of up to three"""
    corpus = pool_segments(n)
    segs = []
    for k in range(n):
        if k % 2:
            segs.append(corpus[k])
            continue
        auds = ["aud-%d" % (k % 11), "www.example.com", "svc-%d" % (k % 7)][:1 + k % 3]
        claims = {"iss": "https://example.com/", "sub": "user-%d" % (k % 37), "aud": auds if k % 4 else auds[0],
                  "exp": CC.T0 + (600 if k % 7 else -600), "iat": CC.T0 - k % 50, "nonce": "abc"}
        segs.append(CC.b64(CC.js(claims)))
    return segs


def pool_values(segs):
    """The distinct sub strings and aud elements (1..64 bytes, a predicate value's bytes) of the payloads, sorted"""
    subs, auds = set(), set()
    for s in segs:
        claims = AC.claims_of(s)
        for key, acc in (("sub", subs), ("aud", auds)):
            v = claims.get(key)
            for e in (v if isinstance(v, list) else [v]):
                if isinstance(e, str) and 0 < len(e.encode()) <= 64 and SM.member_ok(e.encode()):
                    acc.add(e.encode())
    return sorted(subs), sorted(auds)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_in_set_is_the_or_of_equals(ctx, n):
    C = CC.corpus()
    all_profs = [CC.resolve(*C.sets[si]) for si in range(3, 67)]
    segs = set_pool(n)
    arena, spans = pack(segs, lead=3)
    subs, auds = pool_values(set_pool(300))
    assert len(subs) >= 30 and len(auds) >= 16
    subs, auds = subs[::2], auds[::2] + auds[1::2]                          # the first sixteen of each are the members
    reqs = (TC.InSet(P("sub"), 0), TC.ElemIn(P("aud"), 1))
    hits = [0, 0]
    for k in (1, 2, 16):
        ids = load(ctx, [(subs[:k], SM.SEED + k), (auds[:k], k)], first=k % 3)
        for nexpect in (1, 8, 64):
            profs = [CC.resolve(EX, NOW)] + all_profs[:nexpect - 1]
            jobs = [(o, l, i % nexpect) for i, (o, l) in enumerate(spans)]
            got = device_run(ctx, arena, jobs, profs, reqs, ([], [], []), ids)
            assert_host_masks_zero(got, 2)
            ce, me = ctx.claims_match(arena, jobs, profs, [[b"sub"]], [(0, E, v) for v in subs[:k]])
            cl, ml = ctx.claims_match(arena, jobs, profs, [[b"aud"]], [(0, L, v) for v in auds[:k]])
            assert list(ce) == list(cl) == got[0], (k, nexpect)
            want = [(1 if a else 0) | (2 if b else 0) for a, b in zip(me, ml)]
            assert got[1] == want, (k, nexpect, [(i, got[1][i], want[i]) for i in range(n) if got[1][i] != want[i]][:3])
            hits = [hits[0] + sum(m & 1 for m in want), hits[1] + sum(m >> 1 for m in want)]
    if n >= 257:
        assert hits[0] >= 25 and hits[1] >= 25, hits


# ---- (b) ----
@pytest.mark.parametrize("lead", range(4))
def test_directed_list_equals_host_build(ctx, host, lead):
    cases = TC.directed()
    profs = [CC.resolve({}, cases[0][2])]
    segs = [seg for seg, _, _ in cases]
    ops = TC.directed_operands()
    arena, spans = pack(segs, lead=lead, gap=lead % 2)
    jobs = [(o, l, 0) for o, l in spans]
    ids = load(ctx, TC.sets(), first=4 * lead)
    for name, reqs in TC.PRED_SETS.items():
        want = host_run(host, "directed", profs, [(0, s) for s in segs], reqs, ops, TC.sets())
        got = device_run(ctx, arena, jobs, profs, reqs, ops, ids, lead=(lead + 1) % 4)
        assert_same(got, want, (name, lead))
        assert {k for k, c in enumerate(got[0]) if c == _lib.CL_HOST} == TC.directed_hosts()
        if lead == 0:                                                            # ... which is the evaluation on the oracle's map
            base = [c for c in got[0]]
            TC.check(cases, base, got[0], got[1], reqs, ops, TC.sets(), hosts=TC.directed_hosts())


@pytest.fixture(scope="module")
def corpus_want(host):
    """Per corpus group: its profiles, its cases, their operands, the host build's answers and the codes its list
    without the set ops gives.  Computed once; the device runs at the four arena offsets compare with it."""
    C = CC.corpus()
    allc = C.all_cases()
    out = []
    for g, (lo, hi) in enumerate(EC.groups()):
        idx = EC.group_cases(lo, hi)
        profs = [CC.resolve(*C.sets[si]) for si in range(lo, hi)]
        cases = [(allc[k][1] - lo, allc[k][0]) for k in idx]
        per = {}
        for reqs in TC.CORPUS_SETS:
            ops = HC.derive([(seg,) for _, seg in cases], reqs, nstr=1, nnum=0, nhash=0)
            per[reqs] = (ops, host_run(host, "corpus%d" % g, profs, cases, reqs, ops, TC.corpus_sets()))
        out.append((profs, cases, per))
    return out


@pytest.mark.parametrize("lead", range(4))
def test_corpus_equals_host_build(ctx, corpus_want, lead):
    ids = load(ctx, TC.corpus_sets(), first=12)
    hits = 0
    for g, (profs, cases, per) in enumerate(corpus_want):
        arena, spans = pack([seg for _, seg in cases], lead=lead, gap=(lead + g) % 2)
        jobs = [(o, l, p) for (o, l), (p, _) in zip(spans, cases)]
        codes = list(ctx.claims_each(arena, jobs, profs))
        for reqs, (ops, want) in per.items():
            got = device_run(ctx, arena, jobs, profs, reqs, ops, ids, lead=(lead + 1) % 4)
            assert_host_masks_zero(got, len(reqs))
            assert_same(got, want, ("host build", g, lead))
            assert all(a == b or a == _lib.CL_HOST for a, b in zip(got[0], codes))   # only the numeric op's rule changes a code
            only = tuple(r for r in reqs if r[1] >= TC.IN_SET)                       # the set ops alone change none
            c, m = device_run(ctx, arena, jobs, profs, only, ([], [], []), ids)
            assert c == codes, (g, lead)
            hits += sum(1 for x in m if x)
    assert hits >= 500                                                           # two of the groups hold members by the hundred


# ---- (c) ----
def test_wave_mixing_hits_misses_lengths_and_host_tokens(ctx, host):
    s0 = TC.sets()[0]
    pairs = SM.colliding_pairs()
    values = [b"jti-1", b"jti-2", TC.collider(), b"", TC.LONG, TC.LONG_OUT, pairs[0][0], b"revoked-7", TC.LONG + b"y", b"abc", b"ab"]
    segs = []
    for k in range(64):
        v = values[k % len(values)]
        sid = b'"sid":"jti\\u002d1"' if k % 13 == 5 else b'"sid":"' + v + b'"'           # an escape: the host's
        groups = b"[" + b",".join([b'"g%d"' % j for j in range(k % 41)] + ([b'"ops"'] if k % 3 == 0 else [])) + b"]"
        filler = b'"p":"' + b"x" * (330 if k % 9 == 0 else k) + b'",'
        segs.append(CC.b64(b'{"exp":%d,"iat":%d,"iss":"https://example.com/","aud":"www.example.com",' % (CC.T0 + 600, CC.T0 - 900) +
                           filler + sid + b',"groups":' + groups + b',"nonce":"n-%d"}' % k))
    segs[10] = b"e30"
    segs[11] = CC.b64(b'{"exp":%d,"groups":[%s]}' % (CC.T0 + 600, b",".join(b'"g%d"' % j for j in range(40)) + b',"dev"'))
    assert min(len(s) for s in segs) == 3 and any(390 <= len(s) <= 410 for s in segs) and max(len(s) for s in segs) >= 1000
    reqs = (TC.InSet(P("sid"), 0), TC.ElemIn(P("groups"), 1), HC.IsStr(P("sid")), AC.EqA(P("nonce"), 0), TC.InSet(P("sid"), 2),
            MC.Has(P("groups")), TC.InSet(P("groups"), 1))
    ops = ([[b"n-%d" % (k + (k % 5 == 0)) for k in range(64)]], [], [])
    profs = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW), CC.resolve(EX, NOW + 7200 * CC.SECOND)]
    prof = [i % 3 for i in range(64)]
    arena, spans = pack(segs, lead=1)
    jobs = [(o, l, p) for (o, l), p in zip(spans, prof)]
    ids = load(ctx, TC.sets()[:3], first=5)
    got = device_run(ctx, arena, jobs, profs, reqs, ops, ids, lead=3)
    assert_same(got, host_run(host, "wave", profs, list(zip(prof, segs)), reqs, ops, TC.sets()[:3]))
    assert {k for k, c in enumerate(got[0]) if c == _lib.CL_HOST} == {k for k in range(64) if k % 13 == 5 and k not in (10, 11)}
    assert got[0][10] == _lib.CL_NO_TIME and {_lib.CL_OK, _lib.CL_ISS, _lib.CL_EXP} <= set(got[0])
    members = set(s0[0])
    for k, (c, m) in enumerate(zip(*got)):
        if c == _lib.CL_HOST or k in (10, 11):
            continue
        v = values[k % len(values)]
        assert m & 1 == (v in members) and (m >> 1) & 1 == (k % 3 == 0) and (m >> 2) & 1 == 1 and (m >> 6) & 1 == 0, (k, v, hex(m))
        assert (m >> 3) & 1 == (k % 5 != 0) and (m >> 4) & 1 == (v in (b"jti-1", b"jti-2")) and (m >> 5) & 1 == 1, (k, hex(m))
    assert got[1][10] == 0 and got[1][11] == 0b0100010
    assert sum(m & 1 for m in got[1]) >= 20 and sum(1 for c, m in zip(*got) if c != _lib.CL_HOST and not m & 1) >= 20


# ---- (d) ----
def raw_call(ctx, preds, sets, args=None, hargs=None, nsets=None, jobs=((0, 3, 0),), nexpect=1, paths=((b"a", b"b"), (b"c",)),
             arena=b"e30"):
    """One call with poisoned outputs -> (rc, codes + masks as bytes)"""
    n = len(jobs)
    e = _lib.JgExpect()
    e.now_sec = CC.T0
    ps, _k1 = _lib._jg_paths(paths)
    qs, _k2 = _lib._jg_preds(preds)
    ga, _k3 = _lib._jg_args(args) if args is not None else (None, None)
    gh, _k4 = _lib._jg_hargs(hargs) if hargs is not None else (None, None)
    gs = _lib._jg_setargs(sets, nsets) if sets is not None else None
    out = ctypes.create_string_buffer(b"\xee" * n, n)
    m = ctypes.create_string_buffer(b"\xee" * 4 * n, 4 * n)
    rc = _lib.lib().jg_claims_match_set(ctx.h, arena, len(arena), _lib._cjobs(jobs), n, ctypes.byref(e), nexpect,
                                        ctypes.byref(ps), ctypes.byref(qs), None if ga is None else ctypes.byref(ga),
                                        None if gh is None else ctypes.byref(gh), None if gs is None else ctypes.byref(gs),
                                        out, ctypes.cast(m, ctypes.c_void_p))
    return rc, out.raw + m.raw


def test_bad_arguments_and_empty_batch():
    ctx = _lib.Context()                                                         # a context of its own: ids 4..15 are not loaded
    try:
        ex = CC.resolve(EX, NOW)
        for i in range(4):
            ctx.set_load(i, [b"m%d" % i, b"jti-1"], i)
        untouched = (-1, b"\xee" * 5)
        good = (0, bytes([_lib.CL_NO_TIME]) + bytes(4))
        ok = [(0, IN, b"\0"), (1, EL, b"\x03"), (1, IN, b"\0"), (0, IN, b"\x01"), (0, IS, b"")]
        assert raw_call(ctx, ok, [0, 1, 2, 3]) == good
        assert raw_call(ctx, ok, [3, 3, 3, 3]) == good                           # one loaded set under four indices
        assert raw_call(ctx, [(0, IS, b"")], None) == good                       # sets NULL: nsets 0
        assert raw_call(ctx, [(0, IS, b"")], [9, 9], nsets=0) == good            # ... and ids past nsets are not looked at
        assert raw_call(ctx, [(0, IN, b"\0")], [2]) == good
        for preds, sets, nsets in (
                (ok, [0, 1, 2, 3], 5), (ok, [0, 1, 2, 3, 0], None),              # nsets over JG_MAX_SETS
                (ok, [0, 1, 2, 16], None), (ok, [0, 1, 2, 0xffffffff], None),    # an id of 16 or more
                (ok, [0, 1, 2, 4], None), ([], [15], None),                      # an id that is not loaded, asked or not
                ([(0, IN, b"\x04")], [0, 1, 2, 3], None), ([(0, IN, b"\x01")], [0], None), ([(0, EL, b"\xff")], [0, 1], None),
                ([(0, IN, b"\0")], None, None), ([(0, EL, b"\0")], [0], 0),      # no set at all
                ([(0, IN, b"")], [0], None), ([(0, IN, b"\0\0")], [0], None),    # the value is one byte
                ([(0, IN, b"\0"), (1, IN, b"\0"), (0, IN, b"\0")], [0], None),   # the same path, op and set twice
                ([(1, EL, b"\x01"), (1, EL, b"\x01")], [0, 1], None),
                ([(0, 0, b"\0")], [0], None), ([(0, 14, b"\0")], [0], None), ([(0, 255, b"\0")], [0], None),
                ([(2, IN, b"\0")], [0], None), ([(0, EA, b"\0")], [0], None), ([(0, EH, b"\0")], [0], None),
                ([(0, E, b"a\x80")], [0], None), ([(k % 2, IN if k < 8 else EL, bytes([k % 4])) for k in range(17)], [0, 1, 2, 3], None)):
            assert raw_call(ctx, preds, sets, nsets=nsets) == untouched, (preds, sets, nsets)
            assert "jg_claims_match_set" in ctx.error()
        assert raw_call(ctx, ok, [0, 1, 2, 3], jobs=[(0, 3, 1)]) == untouched
        assert raw_call(ctx, ok, [0, 1, 2, 3], jobs=[(1, 3, 0)]) == untouched
        assert raw_call(ctx, ok, [0, 1, 2, 3], nexpect=65) == untouched
        assert raw_call(ctx, ok, [0, 1, 2, 3], paths=[[b"a"], [b"a"]]) == untouched
        assert raw_call(ctx, ok, [0, 1, 2, 3], args=_lib.pack_args([[b"x"]] * 5, [])) == untouched
        # a freed id is not loaded any more
        ctx.set_free(2)
        assert raw_call(ctx, ok, [0, 1, 2, 3]) == untouched and "id 2" in ctx.error()
        assert raw_call(ctx, ok, [0, 1, 3, 3]) == good
        # njobs == 0 returns 0 whatever else is NULL
        assert raw_call(ctx, ok, [0, 1, 3, 3], jobs=[]) == (0, b"")
        assert ctx.claims_match_set(b"", [], [ex], [[b"a"]], [(0, IN, b"\0")], None, None, [7],
                                    null=("paths", "preds", "codes", "masks")) == (b"", [])
        # the older entries keep refusing the new ops
        for op in (12, 13):
            with pytest.raises(_lib.JgError, match="rc=-1"):
                ctx.claims_match(b"e30", [(0, 3, 0)], [ex], [[b"a"]], [(0, op, b"\0")])
            with pytest.raises(_lib.JgError, match="rc=-1"):
                ctx.claims_match_hash(b"e30", [(0, 3, 0)], [ex], [[b"a"]], [(0, op, b"\0")], None, None)
        # then a good call on the same context
        seg = CC.b64(b'{"sid":"jti-1","groups":["x","m3"],"exp":%d}' % (CC.T0 + 600))
        codes, masks = ctx.claims_match_set(seg, [(0, len(seg), 1)], [CC.resolve({}, NOW), ex], [[b"sid"], [b"groups"]],
                                            [(0, IN, b"\0"), (1, EL, b"\x01"), (0, IN, b"\x02"), (1, EL, b"\0"), (0, IS, b"")],
                                            None, None, [0, 3, 1])
        assert codes == bytes([_lib.CL_ISS]) and masks == [0b10111]
    finally:
        ctx.close()


# ---- (e) ----
def test_without_set_ops_equals_claims_match_hash(ctx):
    segs = pool_segments(300)
    arena, spans = pack(segs, lead=1)
    profs = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW)]
    jobs = [(o, l, i % 2) for i, (o, l) in enumerate(spans)]
    strs, nums = AC.derive([(s,) for s in segs], BATCH)
    paths, preds = AC.split(BATCH)
    args = _lib.pack_args(strs, nums, lead=2)
    c, m = ctx.claims_match_hash(arena, jobs, profs, enc(paths), preds, args, None)
    want = (list(c), m)
    ids = load(ctx, TC.sets()[:2])
    for sets in (None, [], ids):                                                  # ... also with sets nobody asks
        c, m = ctx.claims_match_set(arena, jobs, profs, enc(paths), preds, args, None, sets)
        assert (list(c), m) == want
    assert len(set(want[0])) >= 4 and any(want[1])
    # with hash columns too
    reqs = (HC.EqH(P("sub"), 0), HC.IsStr(P("sub")), AC.EqA(P("nonce"), 0))
    s1 = AC.derive([(s,) for s in segs], reqs, nstr=1, nnum=0)[0]
    hashes = [[(HC.source(k, k % 90), 1 + k % 3) for k in range(300)]]
    hp, hq = HC.split(reqs)
    a1, h1 = _lib.pack_args(s1, []), _lib.pack_hargs(hashes)
    c, m = ctx.claims_match_hash(arena, jobs, profs, enc(hp), hq, a1, h1)
    assert ctx.claims_match_set(arena, jobs, profs, enc(hp), hq, a1, h1, ids) == (c, m)


# ---- (f) ----
def test_old_entries_unchanged_around_a_call(ctx):
    segs = set_pool(300)
    arena, spans = pack(segs, lead=2)
    profs = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW)]
    jobs = [(o, l, i % 2) for i, (o, l) in enumerate(spans)]
    names = [n.encode() for n in SC.EIGHT]
    paths, preds = MC.split(MC.FULL)
    astrs, anums = AC.derive([(s,) for s in segs], BATCH)
    apaths, apreds = AC.split(BATCH)

    def old():
        a = ctx.claims_each(arena, jobs, profs, mode="select", names=names)
        b = ctx.claims_paths(arena, jobs, profs, enc(PC.EIGHT))
        return (a[0], bytes(a[1]), bytes(a[2]), b[0], bytes(b[1]), bytes(b[2]), ctx.claims_match(arena, jobs, profs, enc(paths), preds),
                ctx.claims_match_args(arena, jobs, profs, enc(apaths), apreds, _lib.pack_args(astrs, anums)),
                ctx.claims_match_hash(arena, jobs, profs, enc(apaths), apreds, _lib.pack_args(astrs, anums), None),
                ctx.claims_scan(arena, spans, profs[1]), bytes(ctx.claims_extract(arena, spans, profs[0])[1]))
    before = old()
    subs, auds = pool_values(segs)
    ids = load(ctx, [(subs[::2], 1), (auds[::2], 2)], first=9)
    reqs = (TC.InSet(P("sub"), 0), TC.ElemIn(P("aud"), 1), AC.EqA(P("nonce"), 0))
    ops = ([[b"abc"] * 70], [], [])
    small = device_run(ctx, arena, jobs[:70], profs, reqs, ops, ids)             # a smaller batch: the kept buffers are shared
    assert old() == before
    assert device_run(ctx, arena, jobs[:70], profs, reqs, ops, ids) == small
    assert len(set(before[0])) >= 4 and any(m & 1 for m in small[1]) and any(m & 2 for m in small[1])


# ---- (g) ----
def test_replacing_a_set_between_two_scans_changes_the_masks_alone(ctx):
    segs = set_pool(300)
    arena, spans = pack(segs)
    profs = [CC.resolve(EX, NOW), CC.resolve(OTHER, NOW)]
    jobs = [(o, l, i % 2) for i, (o, l) in enumerate(spans)]
    subs, auds = pool_values(segs)
    reqs = (TC.InSet(P("sub"), 0), TC.ElemIn(P("aud"), 1), MC.Has(P("sub")))
    first, second = subs[::2], subs[1::2]
    ctx.set_load(14, first, 5)
    ctx.set_load(15, auds, 6)
    g14, g15 = ctx.set_info(14)["generation"], ctx.set_info(15)["generation"]
    a = device_run(ctx, arena, jobs, profs, reqs, ([], [], []), [14, 15])
    ctx.set_load(14, second, 77)
    b = device_run(ctx, arena, jobs, profs, reqs, ([], [], []), [14, 15])
    assert ctx.set_info(14)["generation"] > g15 > g14 and ctx.set_info(15)["generation"] == g15
    assert a[0] == b[0] and [m & 0b110 for m in a[1]] == [m & 0b110 for m in b[1]]
    decided_sub = [(x & 1, y & 1) for x, y, s in zip(a[1], b[1], segs)
                   if isinstance(AC.claims_of(s).get("sub"), str) and AC.claims_of(s)["sub"].encode() in set(subs) and (x | y) & 0b100]
    assert decided_sub and all(x + y == 1 for x, y in decided_sub)               # every such sub is in exactly one of the halves
    assert any(x for x, _ in decided_sub) and any(y for _, y in decided_sub)
    ctx.set_load(14, first, 1234)                                                # the first set again, under another seed
    assert device_run(ctx, arena, jobs, profs, reqs, ([], [], []), [14, 15]) == a
