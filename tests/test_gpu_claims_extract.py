"""k_claims_extract through the C ABI (jg_claims_extract / Context.claims_extract).

* The whole CPU corpus (tests/claims_corpus.py) and the directed list
  (tests/claims_extract_cases.py), one batch per Expected set: the codes are
  Context.claims_scan's byte for byte, the records the host build's
  (tests/host_unit/claims_extract_test.cpp) byte for byte -- HOST records all
  zero.
* Shapes: every segment length 0..400 at every offset mod 4 with the last job
  ending at arena_len, batches of 1 / 63 / 64 / 65 / 4097 jobs with both outputs
  poisoned, a wave that mixes "e30" and 400-character segments lane by lane, bad
  arguments (vals_out NULL among them), njobs == 0.
* An extract running while a 65,536-job submit of another thread is in flight.
"""
import ctypes
import threading

import pytest

from cap_amd import _lib
from oracle import jws
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import gpu_helpers as H
from tests.test_gpu_claims_scan import EX, NOW, pack, sized_payload

pytestmark = pytest.mark.gpu

POISON = b"\xee" * 64


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """The host build of claims_extract: the reference of the device run."""
    d = tmp_path_factory.mktemp("claims_extract_gpu")
    XC.build_host(str(d / "claims_extract_test"))
    return d, str(d / "claims_extract_test")


def host_records(host_exe, cases, name):
    d, exe = host_exe
    path = str(d / (name + ".txt"))
    XC.write_cases(path, cases)
    return XC.run_host(exe, path)


def records(vals):
    raw = bytes(vals)
    return [raw[64 * k:64 * k + 64] for k in range(len(raw) // 64)]


def device_run(ctx, cases, scan_too=True):
    """cases [(segment, expected, now_ns)] -> (codes, records), one call per Expected set"""
    codes, recs = [None] * len(cases), [None] * len(cases)
    by_set = {}
    for k, (seg, ex, now_ns) in enumerate(cases):
        by_set.setdefault((repr(sorted(ex.items())), now_ns), []).append(k)
    for si, ks in enumerate(by_set.values()):
        arena, spans = pack([cases[k][0] for k in ks], lead=si % 4, gap=1)
        ex = CC.resolve(cases[ks[0]][1], cases[ks[0]][2])
        got, vals = ctx.claims_extract(arena, spans, ex)
        assert len(got) == len(ks) and len(vals) == len(ks)
        if scan_too:
            assert got == ctx.claims_scan(arena, spans, ex)          # the same code, always
        for k, g, r in zip(ks, got, records(vals)):
            codes[k], recs[k] = g, r
    return codes, recs


def assert_same(got, want, cases):
    codes, recs = got
    diff = [k for k in range(len(cases)) if codes[k] != want[0][k] or recs[k] != want[1][k]]
    assert not diff, [(k, codes[k], want[0][k], recs[k].hex(), want[1][k].hex(), cases[k][0]) for k in diff[:3]]


def test_corpus_equals_scan_and_host_build(ctx, host_exe):
    cases = XC.corpus_cases()
    got = device_run(ctx, cases)
    assert_same(got, host_records(host_exe, cases, "corpus"), cases)
    CC.check(got[0])                                   # the oracle's strings; zero HOST on the plain list
    n_host = sum(1 for c, r in zip(*got) if c == _lib.CL_HOST and r == bytes(64))
    assert n_host == got[0].count(_lib.CL_HOST) > 1000


def test_directed_list(ctx, host_exe):
    cases = XC.directed()
    got = device_run(ctx, cases)
    assert_same(got, host_records(host_exe, cases, "directed"), cases)
    assert XC.check_records(cases, got[0], got[1], no_host=True) == len(cases)


def test_every_length_and_alignment(ctx, host_exe):
    """Segments of every length 0..400 at every offset mod 4, the last job ending
    at arena_len: plain payloads where the length allows one, cuts of one
    otherwise (HOST, a zero record)."""
    long = CC.b64(sized_payload(400))
    segs, decided = [], []
    for n in range(401):
        if n >= 136 and n % 4 != 1:
            segs.append(CC.b64(sized_payload(n, n)))
            assert len(segs[-1]) == n
            decided.append(True)
        else:
            segs.append(long[:n])
            decided.append(False)
    cases = [(s, EX, NOW) for s in segs]
    want = host_records(host_exe, cases, "lengths")
    assert all((c != _lib.CL_HOST) == d for c, d in zip(want[0], decided))
    assert XC.check_records(cases, want[0], want[1]) == sum(decided)
    for lead in range(4):
        arena, spans = pack(segs, lead=lead)
        assert spans[-1][0] + spans[-1][1] == len(arena)
        codes, vals = ctx.claims_extract(arena, spans, CC.resolve(EX, NOW))
        assert_same((list(codes), records(vals)), want, cases)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes(ctx, host_exe, n):
    C = CC.corpus()
    pool = C.plain + C.hard[:200]
    segs = [pool[(7 * k) % len(pool)][0] for k in range(n)]
    cases = [(s, EX, NOW) for s in segs]
    arena, spans = pack(segs, lead=3)
    codes, vals = ctx.claims_extract(arena, spans, CC.resolve(EX, NOW))   # both outputs poisoned with 0xee
    recs = records(vals)
    assert len(codes) == n and len(recs) == n
    assert all(c <= _lib.CL_HOST for c in codes) and POISON not in recs
    assert all(r == bytes(64) for c, r in zip(codes, recs) if c == _lib.CL_HOST)
    assert_same((list(codes), recs), host_records(host_exe, cases, "batch%d" % n), cases)
    XC.check_records(cases, list(codes), recs)


def test_wave_mixing_short_and_long_segments(ctx, host_exe):
    long = [CC.b64(sized_payload(400, k)) for k in range(2)]
    segs = [b"e30", long[0], b"e30", long[1]] * 16 + [b"e3", long[0], b"e30"]
    cases = [(s, EX, NOW) for s in segs]
    arena, spans = pack(segs)
    codes, vals = ctx.claims_extract(arena, spans, CC.resolve(EX, NOW))
    recs = records(vals)
    assert_same((list(codes), recs), host_records(host_exe, cases, "wave"), cases)
    assert codes[0] == _lib.CL_NO_TIME and recs[0] == bytes(64)          # {}: decided, nothing present
    assert codes[1] == _lib.CL_OK and codes[3] == _lib.CL_EXP and codes[64] == _lib.CL_HOST
    assert recs[1] != recs[3] and recs[1] == recs[5] and recs[2] == bytes(64)
    XC.check_records(cases, list(codes), recs)


def test_bad_arguments_and_empty_batch(ctx):
    ex = CC.resolve(EX, NOW)
    codes, vals = ctx.claims_extract(b"", [], ex)
    assert codes == b"" and len(vals) == 0
    codes, vals = ctx.claims_extract(b"e30", [(3, 0), (0, 3)], ex)
    assert codes == bytes([_lib.CL_HOST, _lib.CL_NO_TIME]) and bytes(vals) == bytes(128)
    for spans in ([(0, 4)], [(4, 0)], [(2, 2)], [(0, 3), (1 << 40, 1)]):
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.claims_extract(b"e30", spans, ex)
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.claims_extract(b"e30", [(0, 3)], ex, flags=1)
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.claims_extract(b"e30", [(0, 3)], dict(ex, audiences=[b"a"] * 17))
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.claims_extract(b"e30", [(0, 3)], dict(ex, issuer=b"i" * 4000, subject=b"s" * 97))
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.claims_extract(b"e30", [(0, 3)], dict(ex, now_nsec=10 ** 9))
    # vals_out NULL with a job: -1, and nothing is written
    job = (_lib.JgCJob * 1)()
    job[0].off, job[0].len, job[0].flags = 0, 3, 0
    e = _lib.JgExpect()
    e.now_sec = CC.T0
    out = ctypes.create_string_buffer(b"\xee", 1)
    L = _lib.lib()
    assert L.jg_claims_extract(ctx.h, b"e30", 3, job, 1, ctypes.byref(e), out, None) == -1
    assert out.raw == b"\xee"
    vals = (_lib.JgClaims * 1)()
    assert L.jg_claims_extract(ctx.h, b"e30", 3, job, 1, ctypes.byref(e), None, ctypes.cast(vals, ctypes.c_void_p)) == -1
    assert L.jg_claims_extract(ctx.h, b"e30", 3, job, 0, ctypes.byref(e), None, None) == 0      # njobs == 0
    # 16 audiences and 4096 bytes of expected strings are inside the limits
    big = dict(ex, issuer=b"i" * 2048, audiences=[b"a" * 128] * 15 + [b"www.example.com"], subject=b"", id=b"")
    seg = CC.b64(CC.js(dict(CC.STD, iss="i" * 2048)))
    codes, vals = ctx.claims_extract(seg, [(0, len(seg))], big)
    assert codes == bytes([_lib.CL_OK]) and (vals[0].iss_len, vals[0].aud_n) == (2048, 1)
    codes, vals = ctx.claims_extract(b"e30", [(0, 3)], ex)                 # the context still works
    assert codes == bytes([_lib.CL_NO_TIME]) and bytes(vals) == bytes(64)


def test_extract_while_a_submit_is_in_flight():
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
    C = CC.corpus()
    segs = [s for s, _ in C.plain]
    cases = [(s, EX, NOW) for s in segs]
    sarena, spans = pack(segs, lead=1, gap=1)
    c = _lib.Context()
    try:
        c.load_keys([H.abi_key(key)])
        ex = CC.resolve(EX, NOW)
        qc, qv = c.claims_extract(sarena, spans, ex)
        assert XC.check_records(cases, list(qc), records(qv), no_host=True) == len(cases)
        pending = c.submit(arena)
        res = {}
        th = threading.Thread(target=lambda: res.update(out=c.claims_extract(sarena, spans, ex)))
        th.start()
        verdicts = pending.wait()
        th.join()
        assert res["out"][0] == qc and bytes(res["out"][1]) == bytes(qv)
        assert [verdicts[s] for s in slots] == want
    finally:
        c.close()
