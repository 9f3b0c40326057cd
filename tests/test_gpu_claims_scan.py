"""k_claims_scan through the C ABI (jg_claims_scan / Context.claims_scan).

* The whole CPU corpus (tests/claims_corpus.py) in one batch per Expected set
  gives, byte for byte, the codes of the host build of the same decision
  function -- HOST cases included -- and on the plain list the oracle's
  strings with no HOST at all.
* Shapes: every segment length 0..400, every offset mod 4, the last job ending
  at arena_len, batches of 1 / 63 / 64 / 65 / 4097 jobs, a wave that mixes a
  2-byte and a 400-byte segment, poisoned output buffers, bad arguments,
  njobs == 0.
* A scan running while a 65,536-job submit of another thread is in flight.
"""
import threading

import pytest

from cap_amd import _lib
from oracle import jws
from tests import claims_corpus as CC
from tests import gpu_helpers as H

pytestmark = pytest.mark.gpu

EX = {"Issuer": "https://example.com/", "Audiences": ["nope", "www.example.com"]}
NOW = (CC.T0 + 30) * CC.SECOND


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_codes(tmp_path_factory):
    """The host build of claims.hpp on the corpus: the reference of the device run."""
    d = tmp_path_factory.mktemp("claims_scan_gpu")
    CC.write_cases(str(d / "cases.txt"))
    CC.build_host(str(d / "claims_scan_test"))
    return CC.run_host(str(d / "claims_scan_test"), str(d / "cases.txt"))


def pack(segs, lead=0, gap=0):
    """segments -> (arena bytes, spans); `lead` bytes first, `gap` bytes between"""
    buf = bytearray(b"\xaa" * lead)
    spans = []
    for s in segs:
        spans.append((len(buf), len(s)))
        buf += s + b"." * gap
    if gap:
        del buf[len(buf) - gap:]
    return bytes(buf), spans


def device_codes(ctx, cases):
    """cases [(segment, set index)] -> codes, one scan per Expected set"""
    C = CC.corpus()
    out = [None] * len(cases)
    by_set = {}
    for k, (seg, si) in enumerate(cases):
        by_set.setdefault(si, []).append(k)
    for si, ks in by_set.items():
        arena, spans = pack([cases[k][0] for k in ks], lead=si % 4, gap=1)
        got = ctx.claims_scan(arena, spans, CC.resolve(*C.sets[si]))
        assert len(got) == len(ks)
        for k, g in zip(ks, got):
            out[k] = g
    return out


def test_corpus_equals_host_build_and_oracle(ctx, host_codes):
    C = CC.corpus()
    got = device_codes(ctx, C.all_cases())
    diff = [k for k, (g, h) in enumerate(zip(got, host_codes)) if g != h]
    assert not diff, [(k, got[k], host_codes[k], C.all_cases()[k]) for k in diff[:5]]
    CC.check(got)                                   # the oracle's strings; zero HOST on the plain list
    assert _lib.CL_HOST not in got[:len(C.plain)]


def reference(segs, expected, now_ns):
    """oracle code, None where only HOST is right"""
    return [CC.oracle_code(s, expected, now_ns) for s in segs]


def check_against_oracle(got, segs, expected=EX, now_ns=NOW, decided=None):
    want = reference(segs, expected, now_ns)
    for k, (g, w) in enumerate(zip(got, want)):
        if decided is not None and decided[k]:
            assert g == w and g != _lib.CL_HOST, (k, g, w, segs[k])
        else:
            assert g == _lib.CL_HOST or g == w, (k, g, w, segs[k])


def sized_payload(n, k=0):
    """a plain payload whose segment is exactly n characters (n >= 136, n % 4 != 1);
    odd k: expired, even k: valid at NOW"""
    exp = CC.T0 - 600 if k % 2 else CC.T0 + 600
    base = b'{"exp":%d,"iat":%d,"iss":"https://example.com/","aud":"www.example.com","p":"' % (exp, CC.T0 - 900)
    nbytes = n // 4 * 3 + {0: 0, 2: 1, 3: 2}[n % 4]
    return base + b"x" * (nbytes - len(base) - 2) + b'"}'


def test_every_length_and_alignment(ctx):
    """Segments of every length 0..400 at every offset mod 4: plain payloads where
    the length allows one (decided, equal to the oracle), cuts of one otherwise."""
    long = CC.b64(sized_payload(400))
    assert len(long) == 400
    for lead in range(4):
        segs, decided = [], []
        for n in range(401):
            if n >= 136 and n % 4 != 1:
                p = sized_payload(n, n)
                s = CC.b64(p)
                assert len(s) == n
                segs.append(s)
                decided.append(True)
            else:
                segs.append(long[:n])              # a truncated document: HOST
                decided.append(False)
        arena, spans = pack(segs, lead=lead)
        assert spans[-1][0] + spans[-1][1] == len(arena)      # the last job ends at arena_len
        got = ctx.claims_scan(arena, spans, CC.resolve(EX, NOW))
        check_against_oracle(got, segs, decided=decided)
        assert {g for g, d in zip(got, decided) if d} == {_lib.CL_OK, _lib.CL_EXP}
        assert all(g == _lib.CL_HOST for g, d in zip(got, decided) if not d)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes(ctx, n):
    C = CC.corpus()
    segs = [C.plain[(7 * k) % len(C.plain)][0] for k in range(n)]
    arena, spans = pack(segs, lead=3)
    got = ctx.claims_scan(arena, spans, CC.resolve(EX, NOW))       # the binding poisons the output with 0xee
    assert len(got) == n and all(g <= _lib.CL_HOST for g in got)
    check_against_oracle(got, segs, decided=[True] * n)


def test_wave_mixing_short_and_long_segments(ctx):
    long = CC.b64(sized_payload(400))
    segs = [b"e30", long] * 32 + [b"e3", long, b"e30"]        # "{}" beside 400 characters, lane by lane
    arena, spans = pack(segs)
    got = ctx.claims_scan(arena, spans, CC.resolve(EX, NOW))
    check_against_oracle(got, segs)
    assert got[0] == _lib.CL_NO_TIME and got[1] == _lib.CL_OK and got[64] == _lib.CL_HOST


def test_bad_arguments_and_empty_batch(ctx):
    ex = CC.resolve(EX, NOW)
    assert ctx.claims_scan(b"", [], ex) == b""
    assert ctx.claims_scan(b"e30", [(3, 0), (0, 3)], ex) == bytes([_lib.CL_HOST, _lib.CL_NO_TIME])
    for spans in ([(0, 4)], [(4, 0)], [(2, 2)], [(0, 3), (1 << 40, 1)]):
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.claims_scan(b"e30", spans, ex)
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.claims_scan(b"e30", [(0, 3)], ex, flags=1)
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.claims_scan(b"e30", [(0, 3)], dict(ex, audiences=[b"a"] * 17))
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.claims_scan(b"e30", [(0, 3)], dict(ex, issuer=b"i" * 4000, subject=b"s" * 97))
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.claims_scan(b"e30", [(0, 3)], dict(ex, now_nsec=10 ** 9))
    # 16 audiences and 4096 bytes of expected strings are inside the limits
    big = dict(ex, issuer=b"i" * 2048, audiences=[b"a" * 128] * 15 + [b"www.example.com"], subject=b"", id=b"")
    seg = CC.b64(CC.js(dict(CC.STD, iss="i" * 2048)))
    assert ctx.claims_scan(seg, [(0, len(seg))], big) == bytes([_lib.CL_OK])
    assert ctx.claims_scan(b"e30", [(0, 3)], ex) == bytes([_lib.CL_NO_TIME])     # the context still works


def test_scan_while_a_submit_is_in_flight():
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
    sarena, spans = pack(segs, lead=1, gap=1)
    c = _lib.Context()
    try:
        c.load_keys([H.abi_key(key)])
        ex = CC.resolve(EX, NOW)
        quiet = c.claims_scan(sarena, spans, ex)
        check_against_oracle(quiet, segs, decided=[True] * len(segs))
        pending = c.submit(arena)
        res = {}
        th = threading.Thread(target=lambda: res.update(codes=c.claims_scan(sarena, spans, ex)))
        th.start()
        verdicts = pending.wait()
        th.join()
        assert res["codes"] == quiet
        assert [verdicts[s] for s in slots] == want
    finally:
        c.close()
