"""What jg_claims_match_hash runs on the device, on the CPU: the claims scan with
IS_STRING (kernels/claims.hpp, resolved with the hash ops on) and the function
that makes a hashed column's operand (kernels/hash_operand.hpp), built as a
stand-alone program (tests/host_unit/claims_match_hash_test.cpp) and run on the
corpus of tests/claims_corpus.py plus the directed list of
tests/claims_match_hash_cases.py.

* hash_operand() against hashlib + base64: three families x the lengths at which
  either hash takes one block more x source offsets 0..3 mod 4, and family 0.
* Every code is claims_extract's (the corpus list holds one numeric op, whose
  HOST rule is tests/claims_match_args_cases.py's); every decided mask is the
  plain-Python evaluation on the oracle's claims map (oracle.jws._claims_map)
  with that token's operands and sources; every HOST mask is 0.
* With ops 1..9 only and no hash column the program prints
  claims_match_args_test's output.
* resolve_arg_preds() and hash_sources_ok() refuse what the ABI refuses.
* The program built under ASan + UBSan prints the same output.
CPU only; nothing is loaded into Python."""
import os

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_match_args_cases as AC
from tests import claims_match_cases as MC
from tests import claims_match_hash_cases as HC
from tests import claims_paths_cases as PC

P = HC.P
ROWS = [(fam, off, HC.source(n + off, n)) for fam in HC.FAMS for n in HC.LENGTHS for off in range(4)] + \
    [(0, off, HC.source(off, n)) for off, n in enumerate((0, 5, 64, 300))]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("claims_match_hash")
    CC.write_cases(str(d / "cases.txt"))
    XC.write_cases(str(d / "directed.txt"), HC.directed())
    XC.write_cases(str(d / "args_directed.txt"), AC.directed())
    HC.write_operands(str(d / "directed_args.txt"), HC.directed_operands())
    AC.write_operands(str(d / "args_directed_args.txt"), AC.directed_operands())
    HC.build_host(str(d / "claims_match_hash_test"))
    XC.build_host(str(d / "claims_extract_test"))
    return d


@pytest.fixture(scope="module")
def extract_codes(workdir):
    exe = str(workdir / "claims_extract_test")
    return XC.run_host(exe, str(workdir / "cases.txt"))[0], XC.run_host(exe, str(workdir / "directed.txt"))[0]


@pytest.fixture(scope="module")
def corpus_ops():
    cases = XC.corpus_cases()
    return {reqs: HC.derive(cases, reqs) for reqs in HC.CORPUS_SETS}


@pytest.fixture(scope="module")
def corpus_out(workdir, corpus_ops):
    exe, out = str(workdir / "claims_match_hash_test"), {}
    for k, reqs in enumerate(HC.CORPUS_SETS):
        path = str(workdir / ("corpus_args%d.txt" % k))
        HC.write_operands(path, corpus_ops[reqs])
        out[reqs] = HC.run_host(exe, str(workdir / "cases.txt"), path, reqs)
    return out


@pytest.fixture(scope="module")
def directed_out(workdir):
    exe = str(workdir / "claims_match_hash_test")
    return {name: HC.run_host(exe, str(workdir / "directed.txt"), str(workdir / "directed_args.txt"), reqs)
            for name, reqs in HC.PRED_SETS.items()}


@pytest.fixture(scope="module")
def operands_out(workdir):
    return HC.run_operands(str(workdir / "claims_match_hash_test"), ROWS, workdir)


def test_hash_operand_equals_hashlib(operands_out):
    assert len(ROWS) == 3 * 19 * 4 + 4
    for (fam, off, src), got in zip(ROWS, operands_out):
        want = HC.hash_value(src, fam) if fam else b"\0"
        assert got == want, (fam, off, len(src), got, want)
    text = b"".join(operands_out)
    assert b"-" in text and b"_" in text and {len(v) for v in operands_out} == {1, 22, 32, 43}


def test_directed_list(extract_codes, directed_out):
    cases = HC.directed()
    assert _lib.CL_HOST not in extract_codes[1]               # claims_extract alone decides every directed payload
    ops = HC.directed_operands()
    for name, reqs in HC.PRED_SETS.items():
        codes, masks = directed_out[name]
        decided, extra = HC.check(cases, extract_codes[1], codes, masks, reqs, ops)
        assert decided == len(cases) and extra == 0
        assert all(m >> len(reqs) == 0 for m in masks)
    dl, payloads, masks = HC.directed_list(), HC.payloads(), directed_out["HS"][1]
    exp = b',"exp":%d}' % (CC.T0 + 5)

    def bits(member, nth=0):
        ks = [k for k, d in enumerate(dl) if d.member == member]
        assert len(ks) > nth and payloads[ks[nth]] == b"{" + member + exp, (member, ks)
        return masks[ks[nth]] & 0b100011                      # at_hash: present, = hash column 0, is a string

    tok = b"ya29.a0AfH6SMBx-access-token"
    a = HC.hash_value(tok, HC.SHA256)
    q = b'"at_hash":"' + a + b'"'
    assert bits(q) == 0b100001                                # first of that member: no value for the job
    assert bits(b'"at_hash":""') == 0b100001 and bits(b'"at_hash":123') == 0b100000 and bits(b'"at_hash":null') == 0b100000
    assert bits(b'"at_hash":["' + a + b'"]') == 0b100000 and bits(b'"at_hash":{"at_hash":"' + a + b'"}') == 0b100000
    assert bits(b'"x":"' + a + b'"') == 0
    assert bits(q + b',"at_hash":7') == 0b100000 and bits(b'"at_hash":7,' + q) == 0b100011
    wrong = b'"at_hash":"' + HC.hash_value(b"other", HC.SHA256) + b'"'
    assert bits(q + b"," + wrong) == 0b100001 and bits(wrong + b"," + q) == 0b100011
    assert bits(b'"at_hash":"' + a + b'A"') == 0b100001 and bits(b'"at_hash":"' + a[:-1] + b'"') == 0b100001
    # the depths: bits 6 a.b.c.d is a string, 7 = hash column 0, 8 a.b, 9 a.b.c, 10 a
    deep = lambda member: masks[[k for k, d in enumerate(dl) if d.member == member][0]] >> 6
    d4 = b'"a":{"b":{"c":{"d":"' + a + b'"}}}'
    assert deep(b'"a":"s"') == 0b10000 and deep(b'"a":{"b":"s"}') == 0b00100 and deep(b'"a":{"b":{"c":"s"}}') == 0b01000
    assert deep(d4) == 0b00011 and deep(d4 + b',"a":{}') == 0 and deep(b'"a":{},' + d4) == 0b00011
    assert deep(d4 + b',"a":"s"') == 0b10000
    # every family hits on both columns at least once, and misses
    for fam in HC.FAMS:
        ks = [k for k, d in enumerate(dl) if d.h0 and d.h0[1] == fam and d.h1 and d.h1[1] == fam]
        assert any(masks[k] & 0b1010 == 0b1010 for k in ks) and any(masks[k] & 0b1010 == 0 for k in ks)


def test_corpus(extract_codes, corpus_out, corpus_ops):
    cases = XC.corpus_cases()
    base = extract_codes[0]
    for reqs in HC.CORPUS_SETS:
        codes, masks = corpus_out[reqs]
        decided, extra = HC.check(cases, base, codes, masks, reqs, corpus_ops[reqs])
        assert all(m >> len(reqs) == 0 for m in masks)
        assert decided + extra == sum(1 for b in base if b != _lib.CL_HOST) and decided > len(CC.corpus().plain)
        assert extra * 20 <= decided, (extra, decided)
        # every IS_STRING holds on many payloads and fails on many that the scan decides
        for k, (path, op, _) in enumerate(reqs):
            if op != HC.IS_STRING or path == P("deep"):
                continue
            hold = sum((m >> k) & 1 for m in masks)
            fail = sum(1 for c, m in zip(codes, masks) if c != _lib.CL_HOST and not (m >> k) & 1)
            floor = 25 if path in (P("sub"), P("iss")) else 1 if path in (P("aud"), P("x")) else 0   # what the corpus holds
            assert fail >= 100 and hold >= floor, (path, hold, fail)
        assert not any((m >> 2) & 1 for m in masks)           # exp is never a string in a decided payload


def test_old_ops_print_what_claims_match_args_test_prints(workdir, corpus_ops):
    old = str(workdir / "claims_match_args_test")
    AC.build_host(old)
    exe = str(workdir / "claims_match_hash_test")
    for name, reqs in AC.PRED_SETS.items():
        want = AC.run_host(old, str(workdir / "args_directed.txt"), str(workdir / "args_directed_args.txt"), reqs)
        assert AC.run_host(exe, str(workdir / "args_directed.txt"), str(workdir / "args_directed_args.txt"), reqs) == want, name
    cases = XC.corpus_cases()
    for k, reqs in enumerate(AC.CORPUS_SETS):
        path = str(workdir / ("old_corpus_args%d.txt" % k))
        AC.write_operands(path, AC.derive(cases, reqs))
        assert AC.run_host(exe, str(workdir / "cases.txt"), path, reqs) == AC.run_host(old, str(workdir / "cases.txt"), path, reqs)
    # ... also with hash columns that no predicate names
    reqs = AC.NONCE
    s, n = AC.directed_operands()
    idle = [[(b"tok", 1 + k % 3) for k in range(len(s[0]))], [None] * len(s[0])]
    HC.write_operands(str(workdir / "idle_args.txt"), (s, n, idle))
    assert HC.run_host(exe, str(workdir / "args_directed.txt"), str(workdir / "idle_args.txt"), reqs) == \
        AC.run_host(old, str(workdir / "args_directed.txt"), str(workdir / "args_directed_args.txt"), reqs)


def test_resolve_rejects_what_the_abi_rejects(workdir):
    exe, cases, args = str(workdir / "claims_match_hash_test"), str(workdir / "directed.txt"), str(workdir / "directed_args.txt")
    E, H = MC.EQUALS, MC.PRESENT
    EA, GE, EH, IS = AC.EQUALS_ARG, AC.NUM_GE, HC.EQUALS_HASH, HC.IS_STRING
    two = (P("a"), P("b", "c"))
    bad = [
        # the ops outside 1..11
        [(0, 0, b"x")], [(0, 12, b"")], [(0, 12, b"\0")], [(0, 255, b"x")],
        # a hash column index that is not below nhash (the directed operands have two hash columns), a wrong value_len
        [(0, EH, b"\x02")], [(1, EH, b"\xff")], [(0, EH, b"")], [(0, EH, b"\0\0")], [(0, IS, b"x")], [(0, IS, b"\0")],
        # two EQUALS_HASH on the same path and column, two IS_STRING on one path
        [(0, EH, b"\0"), (1, EH, b"\0"), (0, EH, b"\0")], [(0, IS, b""), (0, IS, b"")], [(1, IS, b""), (0, H, b""), (1, IS, b"")],
        # what the entry without hash columns refuses is still refused
        [(0, EA, b"\x01")], [(0, E, b"a\x80")], [(2, IS, b"")], [(k % 2, E, b"v%d" % k) for k in range(17)],
    ]
    for preds in bad:
        assert HC.rejected(exe, cases, args, two, preds) == "preds", preds
    good = [
        [], [(0, EH, b"\0"), (0, EH, b"\x01"), (1, EH, b"\0"), (0, IS, b""), (1, IS, b""), (0, EA, b"\0"), (0, H, b"")],
        [(0, EA, b"\0"), (0, EH, b"\0")],                     # string column 0 and hash column 0 are two columns
        [(0, GE, b"\0" * 8), (0, IS, b"")],
    ]
    for preds in good:
        assert HC.rejected(exe, cases, args, two, preds) is None, preds
    # without hash columns EQUALS_HASH is refused, IS_STRING is not
    AC.write_operands(str(workdir / "plain.txt"), AC.directed_operands())
    assert HC.rejected(exe, str(workdir / "args_directed.txt"), str(workdir / "plain.txt"), two, [(0, EH, b"\0")]) == "preds"
    assert HC.rejected(exe, str(workdir / "args_directed.txt"), str(workdir / "plain.txt"), two, [(0, IS, b"")]) is None
    assert HC.rejected(exe, cases, None, two, [(0, IS, b""), (1, IS, b"")]) is None
    # nhash over JG_MAX_HASH_ARGS; nstr + nhash over JG_MAX_ARGS; the limits themselves
    n = len(HC.directed())
    src = [(b"t", 1)] * n
    for nstr, nhash, want in ((0, 3, "preds"), (3, 2, "preds"), (4, 1, "preds"), (2, 2, None), (3, 1, None), (4, 0, None), (0, 2, None)):
        HC.write_operands(str(workdir / "cols.txt"), ([[b"x"] * n] * nstr, [], [src] * nhash))
        assert HC.rejected(exe, cases, str(workdir / "cols.txt"), two, []) == want, (nstr, nhash)
    # sources: a len over JG_HASH_SRC_MAX or a fam outside 0..3 names the job
    for k, h in ((0, (b"v" * 8193, 1)), (3, (b"v", 4)), (n - 1, (b"", 255))):
        col = [(b"ok", 2)] * n
        col[k] = h
        HC.write_operands(str(workdir / "bad_src.txt"), ([], [], [[None] * n, col]))
        assert HC.rejected(exe, cases, str(workdir / "bad_src.txt"), two, []) == "hsrc %d" % k, (k, h[1])
    col = [(b"v" * 8192, 3)] + [(b"ok", 2)] * (n - 1)
    HC.write_operands(str(workdir / "max_src.txt"), ([], [], [col]))
    assert HC.rejected(exe, cases, str(workdir / "max_src.txt"), two, [(0, EH, b"\0")]) is None


def test_sanitized_build_prints_the_same(workdir, corpus_out, directed_out, operands_out):
    exe = str(workdir / "claims_match_hash_test_asan")
    HC.build_host(exe, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for k, reqs in enumerate(HC.CORPUS_SETS):
        got = HC.run_host(exe, str(workdir / "cases.txt"), str(workdir / ("corpus_args%d.txt" % k)), reqs, env=env)
        assert got == corpus_out[reqs]
    for name, reqs in HC.PRED_SETS.items():
        got = HC.run_host(exe, str(workdir / "directed.txt"), str(workdir / "directed_args.txt"), reqs, env=env)
        assert got == directed_out[name]
    assert HC.run_operands(exe, ROWS, workdir, env=env) == operands_out
