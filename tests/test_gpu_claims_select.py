"""k_claims_select through the C ABI (jg_claims_select / Context.claims_select).
The reference is the host build (tests/host_unit/claims_select_test.cpp), byte
for byte.

* The whole CPU corpus (tests/claims_corpus.py) and the directed list
  (tests/claims_select_cases.py), each for two name sets, one batch per Expected
  set: codes and jg_claims records are Context.claims_extract's on the same
  arena, the jg_selected records the host build's -- HOST records all zero.
* Shapes: every segment length 0..400 at every offset mod 4 with the last job
  ending at arena_len, batches of 1 / 63 / 64 / 65 / 4097 jobs with all three
  outputs poisoned, a wave that mixes "e30" and 400-character segments lane by
  lane, two name sets back to back on one context, bad arguments, njobs == 0.
* A select running while a 65,536-job submit of another thread is in flight.
"""
import ctypes
import threading

import pytest

from cap_amd import _lib
from oracle import jws
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_select_cases as SC
from tests import gpu_helpers as H
from tests.test_gpu_claims_scan import EX, NOW, pack, sized_payload

pytestmark = pytest.mark.gpu

NAMES = ("scope", "roles", "p", "iss")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """The host build of claims_select: the reference of the device run."""
    d = tmp_path_factory.mktemp("claims_select_gpu")
    SC.build_host(str(d / "claims_select_test"))
    return d, str(d / "claims_select_test")


def host_records(host_exe, cases, name, names):
    d, exe = host_exe
    path = str(d / (name + ".txt"))
    XC.write_cases(path, cases)
    return SC.run_host(exe, path, names)


def split(raw, size):
    raw = bytes(raw)
    return [raw[size * k:size * k + size] for k in range(len(raw) // size)]


def enc(names):
    return [n.encode() if isinstance(n, str) else n for n in names]


def device_run(ctx, cases, names, extract_too=True):
    """cases [(segment, expected, now_ns)] -> (codes, jg_claims, jg_selected), one call per Expected set"""
    n = len(cases)
    codes, recs, sels = [None] * n, [None] * n, [None] * n
    by_set = {}
    for k, (seg, ex, now_ns) in enumerate(cases):
        by_set.setdefault((repr(sorted(ex.items())), now_ns), []).append(k)
    for si, ks in enumerate(by_set.values()):
        arena, spans = pack([cases[k][0] for k in ks], lead=si % 4, gap=1)
        ex = CC.resolve(cases[ks[0]][1], cases[ks[0]][2])
        got, vals, sel = ctx.claims_select(arena, spans, ex, enc(names))
        assert len(got) == len(ks) and len(vals) == len(ks) and len(sel) == len(ks)
        if extract_too:                                              # the same code and record, always
            xc, xv = ctx.claims_extract(arena, spans, ex)
            assert got == xc and bytes(vals) == bytes(xv)
        for k, g, r, q in zip(ks, got, split(vals, 64), split(sel, 80)):
            codes[k], recs[k], sels[k] = g, r, q
    return codes, recs, sels


def assert_same(got, want, cases):
    diff = [k for k in range(len(cases)) if any(got[j][k] != want[j][k] for j in range(3))]
    assert not diff, [(k, got[0][k], want[0][k], got[1][k].hex(), want[1][k].hex(), got[2][k].hex(), want[2][k].hex(),
                       cases[k][0]) for k in diff[:3]]


@pytest.mark.parametrize("names", [SC.CORPUS_NAMES, SC.EIGHT], ids=["corpus-keys", "eight"])
def test_corpus_equals_extract_and_host_build(ctx, host_exe, names):
    cases = XC.corpus_cases()
    got = device_run(ctx, cases, names)
    assert_same(got, host_records(host_exe, cases, "corpus", names), cases)
    CC.check(got[0])                                   # the oracle's strings; zero HOST on the plain list
    SC.check_selected(cases, got[0], got[2], names)
    n_host = sum(1 for c, q in zip(got[0], got[2]) if c == _lib.CL_HOST and q == bytes(80))
    assert n_host == got[0].count(_lib.CL_HOST) > 1000


@pytest.mark.parametrize("names", [SC.EIGHT, ("scope", "scopes", "s")], ids=["eight", "prefixes"])
def test_directed_list(ctx, host_exe, names):
    cases = SC.directed() + SC.host_only()
    got = device_run(ctx, cases, names)
    assert_same(got, host_records(host_exe, cases, "directed", names), cases)
    n = len(cases) - 1
    assert SC.check_selected(cases[:n], got[0][:n], got[2][:n], names, no_host=True) == n
    assert got[0][n] == _lib.CL_HOST and got[2][n] == bytes(80)


def sized_select_payload(n, k=0):
    """sized_payload(n, k) with selected members (a string, an array, the padding
    string itself) where the length allows them"""
    plain = sized_payload(n, k)
    head = b'{"scope":"a b%s","roles":["r",{"k":[%d]}],' % (b"c" * (k % 2), k % 10)    # odd k: other spans
    pad = len(plain) - (plain.index(b'"p":"') + 5) - 2  # the x's of sized_payload's padding member
    if pad < len(head) - 1:                            # no room for the members
        return plain
    out = head + plain[1:len(plain) - 2 - (len(head) - 1)] + b'"}'          # len(head) - 1 fewer bytes of padding
    assert len(out) == len(plain)
    return out


def test_every_length_and_alignment(ctx, host_exe):
    """Segments of every length 0..400 at every offset mod 4, the last job ending
    at arena_len: plain payloads (with selected members from the length that has
    room for them) where the length allows one, cuts of one otherwise (HOST, zero
    records)."""
    long = CC.b64(sized_select_payload(400))
    assert len(long) == 400
    segs, decided = [], []
    for n in range(401):
        if n >= 136 and n % 4 != 1:
            segs.append(CC.b64(sized_select_payload(n, n)))
            assert len(segs[-1]) == n
            decided.append(True)
        else:
            segs.append(long[:n])
            decided.append(False)
    cases = [(s, EX, NOW) for s in segs]
    want = host_records(host_exe, cases, "lengths", NAMES)
    assert all((c != _lib.CL_HOST) == d for c, d in zip(want[0], decided))
    assert SC.check_selected(cases, want[0], want[2], NAMES) == sum(decided)
    with_member = sum(1 for q in want[2] if SC.unpack(q)["type"][1] == _lib.SEL_ARRAY)
    assert 100 < with_member < sum(decided)            # both shapes are there
    for lead in range(4):
        arena, spans = pack(segs, lead=lead)
        assert spans[-1][0] + spans[-1][1] == len(arena)
        codes, vals, sel = ctx.claims_select(arena, spans, CC.resolve(EX, NOW), enc(NAMES))
        assert_same((list(codes), split(vals, 64), split(sel, 80)), want, cases)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes(ctx, host_exe, n):
    C = CC.corpus()
    pool = C.plain + C.hard[:200] + [(c[0], 0) for c in SC.directed()]
    segs = [pool[(7 * k) % len(pool)][0] for k in range(n)]
    cases = [(s, EX, NOW) for s in segs]
    arena, spans = pack(segs, lead=3)
    names = SC.EIGHT
    codes, vals, sel = ctx.claims_select(arena, spans, CC.resolve(EX, NOW), enc(names))   # all outputs poisoned with 0xee
    recs, sels = split(vals, 64), split(sel, 80)
    assert len(codes) == n and len(recs) == n and len(sels) == n
    assert all(c <= _lib.CL_HOST for c in codes)
    assert b"\xee" * 64 not in recs and not any(b"\xee" * 4 in q for q in sels)          # no poison survives
    assert all(r == bytes(64) and q == bytes(80) for c, r, q in zip(codes, recs, sels) if c == _lib.CL_HOST)
    assert_same((list(codes), recs, sels), host_records(host_exe, cases, "batch%d" % n, names), cases)
    SC.check_selected(cases, list(codes), sels, names)


def test_wave_mixing_short_and_long_segments(ctx, host_exe):
    long = [CC.b64(sized_select_payload(400, k)) for k in range(2)]
    segs = [b"e30", long[0], b"e30", long[1]] * 16 + [b"e3", long[0], b"e30"]
    cases = [(s, EX, NOW) for s in segs]
    arena, spans = pack(segs)
    codes, vals, sel = ctx.claims_select(arena, spans, CC.resolve(EX, NOW), enc(NAMES))
    got = (list(codes), split(vals, 64), split(sel, 80))
    assert_same(got, host_records(host_exe, cases, "wave", NAMES), cases)
    assert codes[0] == _lib.CL_NO_TIME and got[2][0] == bytes(80)           # {}: decided, nothing present
    assert codes[1] == _lib.CL_OK and codes[3] == _lib.CL_EXP and codes[64] == _lib.CL_HOST
    assert got[2][1] != got[2][3] and got[2][1] == got[2][5] and got[2][2] == bytes(80)
    assert list(SC.unpack(got[2][1])["type"][:4]) == [_lib.SEL_STRING, _lib.SEL_ARRAY, _lib.SEL_STRING, _lib.SEL_STRING]
    SC.check_selected(cases, got[0], got[2], NAMES)


def test_two_name_sets_back_to_back(ctx, host_exe):
    """The kept device buffer of the names: a second call with fewer, shorter and
    other names sees nothing of the first."""
    cases = SC.directed()
    first, second = SC.EIGHT, ("s",)
    a = device_run(ctx, cases, first, extract_too=False)
    b = device_run(ctx, cases, second, extract_too=False)
    c = device_run(ctx, cases, (), extract_too=False)
    d = device_run(ctx, cases, first, extract_too=False)
    assert_same(a, host_records(host_exe, cases, "b2b_first", first), cases)
    assert_same(b, host_records(host_exe, cases, "b2b_second", second), cases)
    assert set(c[2]) == {bytes(80)}                                         # no names: every slot ABSENT
    assert a == d
    assert any(SC.unpack(q)["type"][0] for q in b[2])
    assert all(SC.unpack(q)["type"][1:] == (0,) * 7 for q in b[2])          # slots 1..7 of the first set are gone


def test_bad_arguments_and_empty_batch(ctx):
    ex = CC.resolve(EX, NOW)
    good = [b"scope"]
    codes, vals, sel = ctx.claims_select(b"", [], ex, good)
    assert codes == b"" and len(vals) == 0 and len(sel) == 0
    codes, vals, sel = ctx.claims_select(b"e30", [(3, 0), (0, 3)], ex, good)
    assert codes == bytes([_lib.CL_HOST, _lib.CL_NO_TIME]) and bytes(vals) == bytes(128) and bytes(sel) == bytes(160)
    for spans in ([(0, 4)], [(4, 0)], [(2, 2)], [(0, 3), (1 << 40, 1)]):
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.claims_select(b"e30", spans, ex, good)
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.claims_select(b"e30", [(0, 3)], ex, good, flags=1)
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.claims_select(b"e30", [(0, 3)], dict(ex, audiences=[b"a"] * 17), good)
    # every bad select: -1 and the three outputs unwritten
    L = _lib.lib()
    job = (_lib.JgCJob * 1)()
    job[0].off, job[0].len, job[0].flags = 0, 3, 0
    e = _lib.JgExpect()
    e.now_sec = CC.T0

    def raw_call(names, n=None, select=True, code=True, vals=True, sels=True, njobs=1):
        blob = b"".join(names)
        keep = ctypes.create_string_buffer(blob, max(1, len(blob)))
        s = _lib.JgSelect()
        s.names = ctypes.cast(keep, ctypes.c_void_p)
        s.n = len(names) if n is None else n
        for k, x in enumerate(names[:_lib.MAX_SELECT]):
            s.name_len[k] = len(x)
        out = ctypes.create_string_buffer(b"\xee", 1)
        v = ctypes.create_string_buffer(b"\xee" * 64, 64)
        q = ctypes.create_string_buffer(b"\xee" * 80, 80)
        rc = L.jg_claims_select(ctx.h, b"e30", 3, job, njobs, ctypes.byref(e), ctypes.byref(s) if select else None,
                                out if code else None, v if vals else None, q if sels else None)
        return rc, out.raw + v.raw + q.raw
    untouched = b"\xee" * 145
    bad = [
        [b"n%d" % k for k in range(9)],                      # n > JG_MAX_SELECT
        [b""], [b"scope", b""],                              # a name of length 0
        [b"L" * 65],                                         # longer than JG_SELECT_NAME_MAX
        [b"a\x1fb"], [b"a\x7fb"], [b"a\x80b"], [b"a\x00b"],  # a byte outside 0x20..0x7e
        [b'a"b'], [b"a\\b"],
        [b"scope", b"scope"], [b"a", b"b", b"a"],            # two equal names
    ]
    for names in bad:
        assert raw_call(names) == (-1, untouched), names
    assert raw_call([b"a"], n=0xffffffff) == (-1, untouched)
    assert raw_call(good, select=False) == (-1, untouched)
    assert raw_call(good, sels=False) == (-1, untouched)
    assert raw_call(good, vals=False) == (-1, untouched)
    assert raw_call(good, code=False) == (-1, untouched)
    assert raw_call(good, select=False, code=False, vals=False, sels=False, njobs=0) == (0, untouched)   # njobs == 0
    rc, out = raw_call([b"L" * 64, b" ~"])                   # inside the limits
    assert rc == 0 and out == bytes([_lib.CL_NO_TIME]) + bytes(144)
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.claims_select(b"e30", [(0, 3)], ex, [b"x"] * 2)
    # then a good call on the same context
    seg = CC.b64(b'{"scope":"a","exp":%d}' % (CC.T0 + 600))
    codes, vals, sel = ctx.claims_select(seg, [(0, len(seg))], ex, [b"nope", b"scope"])
    assert codes == bytes([_lib.CL_ISS])
    assert (sel[0].off[1], sel[0].len[1], sel[0].type[1], sel[0].type[0]) == (10, 1, _lib.SEL_STRING, _lib.SEL_ABSENT)


def test_select_while_a_submit_is_in_flight(host_exe):
    keys, toks = H.golden()
    kid = "p256-a"
    key = next(k for k in keys if k["kid"] == kid)
    sel = [t for t in toks if t["key"] == kid and t["alg"] == "ES256"
           and (t["name"].startswith("valid-") or t["name"].startswith("tamper-sig"))][:16]
    assert sel
    okey = jws.Key.from_fixture(key)
    want_one = [int(jws.verify_sig(jws.parse_jws(t["token"]), okey)) for t in sel]
    assert 1 in want_one
    reps = 65536 // len(sel) + 1
    tiled = (sel * reps)[:65536]
    arena, slots = H.jobs_from_tokens(tiled, {kid: 0})
    want = (want_one * reps)[:65536]
    cases = [(s, EX, NOW) for s, _, _ in SC.directed()] + [(s, EX, NOW) for s, _ in CC.corpus().plain]
    names = SC.EIGHT
    sarena, spans = pack([c[0] for c in cases], lead=1, gap=1)
    ref = host_records(host_exe, cases, "inflight", names)
    c = _lib.Context()
    try:
        c.load_keys([H.abi_key(key)])
        ex = CC.resolve(EX, NOW)
        qc, qv, qs = c.claims_select(sarena, spans, ex, enc(names))
        assert_same((list(qc), split(qv, 64), split(qs, 80)), ref, cases)
        pending = c.submit(arena)
        res = {}
        th = threading.Thread(target=lambda: res.update(out=c.claims_select(sarena, spans, ex, enc(names))))
        th.start()
        verdicts = pending.wait()
        th.join()
        assert res["out"][0] == qc and bytes(res["out"][1]) == bytes(qv) and bytes(res["out"][2]) == bytes(qs)
        assert [verdicts[s] for s in slots] == want
    finally:
        c.close()
