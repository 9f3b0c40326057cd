"""The claims scan with per-token operands and numeric tests (kernels/claims.hpp
claims_match_args) on the CPU: the code k_claims_match_args runs, built as a
stand-alone program (tests/host_unit/claims_match_args_test.cpp) and run on the
corpus of tests/claims_corpus.py plus the directed list of
tests/claims_match_args_cases.py.

* Every code is claims_extract's, or JG_CL_HOST where the full path of a numeric
  predicate reaches a number that is not -?(0|[1-9][0-9]{0,14}).  On the directed
  list those cases are named one by one and claims_extract decides every payload;
  on the corpus they are exactly the ones a Python evaluation of the rule on the
  payload's text names.
* Every non-HOST mask is the plain-Python evaluation on the oracle's claims map
  (oracle.jws._claims_map) with that token's operands; every HOST mask is 0.
* On the corpus the operands are derived from the token index (the true value,
  its last byte changed, its first byte changed, a proper prefix, one byte more,
  ""), and each ARG predicate holds on at least 25 payloads and fails on at least
  100 whose value is a string (a sixth of the operands are the true value).
* With ops 1..4 only the program prints claims_match_test's output.
* resolve_arg_preds() and arg_operands_ok() refuse what the ABI refuses.
* The program built under ASan + UBSan prints the same output.
CPU only; nothing is loaded into Python."""
import os
import struct

import pytest

from cap_amd import _lib
from oracle import jws
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_match_args_cases as AC
from tests import claims_match_cases as MC
from tests import claims_paths_cases as PC

P = AC.P


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("claims_match_args")
    CC.write_cases(str(d / "cases.txt"))
    XC.write_cases(str(d / "directed.txt"), AC.directed())
    XC.write_cases(str(d / "old_directed.txt"), MC.directed())
    AC.write_operands(str(d / "directed_args.txt"), AC.directed_operands())
    AC.build_host(str(d / "claims_match_args_test"))
    XC.build_host(str(d / "claims_extract_test"))
    return d


@pytest.fixture(scope="module")
def extract_codes(workdir):
    exe = str(workdir / "claims_extract_test")
    return XC.run_host(exe, str(workdir / "cases.txt"))[0], XC.run_host(exe, str(workdir / "directed.txt"))[0]


@pytest.fixture(scope="module")
def corpus_ops():
    cases = XC.corpus_cases()
    return {reqs: AC.derive(cases, reqs) for reqs in AC.CORPUS_SETS}


@pytest.fixture(scope="module")
def corpus_out(workdir, corpus_ops):
    exe, out = str(workdir / "claims_match_args_test"), {}
    for k, reqs in enumerate(AC.CORPUS_SETS):
        path = str(workdir / ("corpus_args%d.txt" % k))
        AC.write_operands(path, corpus_ops[reqs])
        out[reqs] = AC.run_host(exe, str(workdir / "cases.txt"), path, reqs)
    return out


@pytest.fixture(scope="module")
def directed_out(workdir):
    exe = str(workdir / "claims_match_args_test")
    return {name: AC.run_host(exe, str(workdir / "directed.txt"), str(workdir / "directed_args.txt"), reqs)
            for name, reqs in AC.PRED_SETS.items()}


def test_directed_list(extract_codes, directed_out):
    cases = AC.directed()
    # claims_extract alone decides every directed payload: nothing is HOST but what the list names
    assert _lib.CL_HOST not in extract_codes[1]
    ops = AC.directed_operands()
    for name, reqs in AC.PRED_SETS.items():
        codes, masks = directed_out[name]
        hosts = AC.directed_hosts(name)
        decided, extra = AC.check(cases, extract_codes[1], codes, masks, reqs, ops, hosts=hosts)
        assert decided == len(cases) - len(hosts) and extra == len(hosts)
        assert [k for k, c in enumerate(codes) if c == _lib.CL_HOST] == sorted(hosts)
        assert all(m >> len(reqs) == 0 for m in masks)
    assert len(AC.directed_hosts("AUTH")) == 10 and len(AC.directed_hosts("EXPNUM")) == 2
    assert len(AC.directed_hosts("MIXED")) == 11
    assert not AC.directed_hosts("NONCE") and not AC.directed_hosts("DEEP") and not AC.directed_hosts("EMPTY")
    assert set(directed_out["EMPTY"][1]) == {0}
    payloads = AC.payloads()
    exp = b',"exp":%d}' % (CC.T0 + 5)
    dl = AC.directed_list()

    def bits(name, member, **kw):
        ks = [k for k, d in enumerate(dl) if d.member == member and all(getattr(d, a) == v for a, v in kw.items())]
        assert len(ks) == 1 and payloads[ks[0]] == b"{" + member + exp, (member, kw, ks)
        return directed_out[name][1][ks[0]]
    # NONCE: 0 = s0, 1 = "abc", 2 = s1, 3 present
    for n in AC.LENGTHS:
        assert bits("NONCE", b'"nonce":"' + AC.ABC[:n] + b'"', s0=AC.ABC[:n], s1=AC.flip(AC.ABC[:n], n - 1) if n else b"x") == (0b1011 if n == 3 else 0b1001)
    for n in (5, 8, 64):
        for k in sorted({0, 3, 4, n - 1}):
            assert bits("NONCE", b'"nonce":"' + AC.ABC[:n] + b'"', s0=AC.flip(AC.ABC[:n], k)) == 0b1100
    assert bits("NONCE", b'"nonce":"abc"', s0=b"abc", s1=b"abc") == 0b1111
    assert bits("NONCE", b'"nonce":"abc"', s0=b"abd") == 0b1010
    assert bits("NONCE", b'"nonce":"n1","nonce":"n2"') == 0b1100 and bits("NONCE", b'"nonce":"n2","nonce":"n1"') == 0b1001
    assert bits("NONCE", b'"nonce":"n1","nonce":7') == 0b1000 and bits("NONCE", b'"nonce":7,"nonce":"n1"') == 0b1101
    assert bits("NONCE", b'"nonce":["abc"]') == 0b1000 and bits("NONCE", b'"nonce":""', s0=b"x") == 0b1100
    assert bits("NONCE", b'"nonce":"ab\xffc"') == 0b1000
    assert bits("NONCE", b'"nonce":"' + AC.ABC + b'x"') == 0b1000
    # DEEP: 0 cnf.jkt = s0, 1 cnf present, 2 a.b.c.d = s1, 3 = "deep", 4 has z
    jkt = b"0ZcOCORZNYy-DWpqq30jZyJGHTN0d2HglBV3uiguA4I"
    assert bits("DEEP", b'"cnf":{"jkt":"' + jkt + b'"}', s0=jkt) == 0b00011
    assert bits("DEEP", b'"cnf":{"jkt":"' + jkt + b'"}', s0=AC.flip(jkt, 42)) == 0b00010
    assert bits("DEEP", b'"cnf":{"jkt":"' + jkt + b'"},"cnf":{}') == 0b00010              # a repeated parent
    assert bits("DEEP", b'"cnf":{},"cnf":{"jkt":"' + jkt + b'"}') == 0b00011
    assert bits("DEEP", b'"a":{"b":{"c":{"d":"deep"}}}', s1=b"deep") == 0b01100
    assert bits("DEEP", b'"a":{"b":{"c":{"d":"deep"},"c":{}}}') == 0
    assert bits("DEEP", b'"a":{"b":{"c":{"d":["z","deep"]}}}') == 0b10000
    # AUTH: 0 >= n0, 1 <= n0, 2 >= 1000, 3 <= 1000, 4 present, 5 >= n1, 6 <= n1, 7 frac present
    for lit, v in ((b"0", 0), (b"-0", 0), (b"-1", -1)):
        assert bits("AUTH", b'"auth_time":' + lit, n0=v, n1=v + 1) == 0b01011011
        assert bits("AUTH", b'"auth_time":' + lit, n0=v - 1, n1=v) == 0b01111001
        assert bits("AUTH", b'"auth_time":' + lit, n0=v + 1, n1=v - 1) == 0b00111010
    assert bits("AUTH", b'"auth_time":1000', n0=1000, n1=1001) == 0b01011111
    big = 999999999999999
    assert bits("AUTH", b'"auth_time":%d' % big, n0=big) == 0b01010111
    assert bits("AUTH", b'"auth_time":%d' % big, n0=AC.INT64_MAX) == 0b00110110
    assert bits("AUTH", b'"auth_time":-%d' % big, n0=AC.INT64_MIN) == 0b01011001
    assert bits("AUTH", b'"auth_time":"123"') == 0b00010000 and bits("AUTH", b'"auth_time":[5]') == 0b00010000
    assert bits("AUTH", b'"auth_time":null') == 0b00010000
    assert bits("AUTH", b'"frac":0.5') == 0b10000000                                      # only PRESENT on the path
    assert bits("AUTH", b'"auth_time":5,"auth_time":6') == 0b01111001                    # the last member: 6
    # EXPNUM: 0 exp >= T0, 1 exp <= n0, 2 a.b.c.n >= 5, 3 a.n <= n1, 4 frac present; the registered logic is unchanged
    assert bits("EXPNUM", b'"a":{"n":3,"b":{"c":{"n":5}}}') == 0b01101
    assert bits("EXPNUM", b'"a":{"n":3,"b":{"c":{"n":4}}}') == 0b00001
    assert bits("EXPNUM", b'"auth_time":0', n0=AC.INT64_MIN) == 0b00001
    assert bits("EXPNUM", b'"auth_time":%d' % big, n0=AC.INT64_MAX) == 0b00011
    k = [i for i, d in enumerate(dl) if d.member.startswith(b'"nonce":"n-0.S6_WzA2Mj","auth_time":%d' % (CC.T0 - 30))][0]
    assert directed_out["MIXED"][1][k] == 0b1101111111


def test_corpus(extract_codes, corpus_out, corpus_ops):
    cases = XC.corpus_cases()
    nplain = len(CC.corpus().plain)
    base = extract_codes[0]
    for reqs in AC.CORPUS_SETS:
        codes, masks = corpus_out[reqs]
        decided, extra = AC.check(cases, base, codes, masks, reqs, corpus_ops[reqs])
        assert all(m >> len(reqs) == 0 for m in masks)
        numeric = any(op in AC.NUMERIC for _, op, _ in reqs)
        # The cap on the extra HOST share is the rule's own count: check() has held every extra HOST case to the
        # Python evaluation of the rule and every case the rule names to HOST.  A list without a numeric op has none.
        want = sum(1 for case, b in zip(cases, base) if b != _lib.CL_HOST and AC.rule_sends_to_host(XC.payload_of(case[0]), reqs))
        assert extra == want and (numeric or extra == 0)
        assert decided + extra == sum(1 for b in base if b != _lib.CL_HOST) and decided > nplain
        assert extra * 20 <= decided, (extra, decided)                   # ... and it stays a small share
        # each ARG predicate holds on many payloads and fails on many whose value is a string
        strs = corpus_ops[reqs][0]
        for k, (path, op, col) in enumerate(reqs):
            if op != AC.EQUALS_ARG:
                continue
            hold = fail = 0
            for case, code, mask in zip(cases, codes, masks):
                if code == _lib.CL_HOST:
                    continue
                present, v = PC.walk(AC.claims_of(case[0]), path)
                hold += (mask >> k) & 1
                fail += present and isinstance(v, str) and not (mask >> k) & 1
            if k < 3:                                                   # sub, jti, iss: the column is derived from this path
                assert hold >= 25 and fail >= 100, (path, hold, fail)
        if numeric:
            for k, (path, op, _) in enumerate(reqs):
                if op in AC.NUMERIC and path[0] in ("exp", "iat", "nbf"):
                    n1 = sum((m >> k) & 1 for m in masks)
                    n0 = sum(1 for c, m in zip(codes, masks) if c != _lib.CL_HOST and not (m >> k) & 1)
                    assert n1 >= 100 and n0 >= 100, (path, op, n1, n0)


def test_old_ops_print_what_claims_match_test_prints(workdir):
    old = str(workdir / "claims_match_test")
    MC.build_host(old)
    exe = str(workdir / "claims_match_args_test")
    for cases, sets in (("old_directed.txt", AC.OLD_SETS), ("cases.txt", MC.CORPUS_SETS)):
        for reqs in sets:
            want = MC.run_host(old, str(workdir / cases), reqs)
            assert AC.run_host(exe, str(workdir / cases), None, reqs) == want
    # ... also with operand columns that no predicate names
    reqs = MC.SCOPE
    ops = AC.derive(MC.directed(), reqs)
    AC.write_operands(str(workdir / "idle_args.txt"), ops)
    assert AC.run_host(exe, str(workdir / "old_directed.txt"), str(workdir / "idle_args.txt"), reqs) == \
        MC.run_host(old, str(workdir / "old_directed.txt"), reqs)


def test_resolve_rejects_what_the_abi_rejects(workdir):
    exe, cases, args = str(workdir / "claims_match_args_test"), str(workdir / "directed.txt"), str(workdir / "directed_args.txt")
    E, W, L, H = MC.EQUALS, MC.HAS_WORD, MC.HAS_ELEMENT, MC.PRESENT
    EA, GE, LE, GA, LA = AC.EQUALS_ARG, AC.NUM_GE, AC.NUM_LE, AC.NUM_GE_ARG, AC.NUM_LE_ARG
    q = lambda n: struct.pack("<q", n)
    two = (P("a"), P("b", "c"))
    bad = [
        # everything resolve_preds refuses
        [(k % 2, L, b"v%d" % k) for k in range(17)], [(2, E, b"x")], [(0, E, b"x"), (255, H, b"")],
        [(0, 0, b"x")], [(0, 10, b"\0")], [(0, 255, b"x")],
        [(0, E, b"v" * 65)], [(0, W, b"")], [(0, L, b"")], [(0, H, b"x")], [(0, E, b"a\x1fb")], [(1, L, b"a\x80b")],
        [(0, E, b'a"b')], [(1, W, b"a\\b")], [(0, W, b"a b")], [(0, E, b"x"), (0, E, b"x")],
        # a column index past its count (the directed operands have two columns of each kind)
        [(0, EA, b"\x02")], [(0, GA, b"\x02")], [(1, LA, b"\x04")], [(0, EA, b"\xff")],
        # a wrong value_len
        [(0, EA, b"")], [(0, EA, b"\0\0")], [(0, GA, b"")], [(0, LA, b"\0\0")], [(0, GE, b"")], [(0, GE, q(1)[:7])],
        [(0, LE, q(1) + b"\0")], [(0, GE, b"\x01")],
        # the same path, op and column (or bound)
        [(0, EA, b"\0"), (1, EA, b"\0"), (0, EA, b"\0")], [(1, GA, b"\x01"), (1, GA, b"\x01")],
        [(0, LA, b"\0"), (0, GE, q(5)), (0, LA, b"\0")], [(0, GE, q(5)), (0, GE, q(5))], [(1, LE, q(-1)), (1, LE, q(-1))],
    ]
    for preds in bad:
        assert AC.rejected(exe, cases, args, two, preds) == "preds", preds
    # without columns every ARG op is refused, and more than JG_MAX_ARGS columns are
    for preds in ([(0, EA, b"\0")], [(0, GA, b"\0")], [(0, LA, b"\0")]):
        assert AC.rejected(exe, cases, None, two, preds) == "preds", preds
    n = len(AC.directed())
    AC.write_operands(str(workdir / "five_s.txt"), ([[b"x"] * n] * 5, []))
    AC.write_operands(str(workdir / "five_n.txt"), ([], [[0] * n] * 5))
    assert AC.rejected(exe, cases, str(workdir / "five_s.txt"), two, []) == "preds"
    assert AC.rejected(exe, cases, str(workdir / "five_n.txt"), two, []) == "preds"
    for paths in ([P("n%d" % k) for k in range(9)], [P()], [P("a", "b", "c", "d", "e")], [P("a"), P("a")]):
        assert AC.rejected(exe, cases, args, paths, []) == "paths", paths
    good = [
        [], [(0, EA, b"\0"), (0, EA, b"\x01"), (1, EA, b"\0"), (0, E, b"\0".hex().encode())],
        [(0, GA, b"\0"), (0, LA, b"\0"), (0, GA, b"\x01"), (0, GE, q(0)), (0, LE, q(0)), (0, GE, q(1)), (1, GE, q(0))],
        [(0, GE, q(AC.INT64_MIN)), (0, LE, q(AC.INT64_MAX)), (0, GE, b'"\\\x00\x80\xff\x1f\x7f ')],   # a bound's bytes are no text
        [(k % 2, (GE, LE)[k // 4], q(k)) for k in range(8)] + [(k % 2, EA, bytes([k // 2])) for k in range(4)] +
        [(0, GA, b"\0"), (0, LA, b"\0"), (1, GA, b"\x01"), (1, LA, b"\x01")],        # sixteen
    ]
    for preds in good:
        assert AC.rejected(exe, cases, args, two, preds) is None, preds
    # the limits themselves: four columns of each kind, operands of 64 bytes
    AC.write_operands(str(workdir / "four.txt"), ([[b"v" * 64] * n] * 4, [[AC.INT64_MIN] * n] * 4))
    assert AC.rejected(exe, cases, str(workdir / "four.txt"), two, [(0, EA, b"\x03"), (1, LA, b"\x03")]) is None
    # operands: a len over JG_PRED_VALUE_MAX or a refused byte names the job
    for k, v in ((0, b"v" * 65), (3, b"a\x1fb"), (n - 1, b"a\x7fb"), (5, b"\x80"), (1, b'a"'), (2, b"\\"), (4, b"a\0")):
        col = [b"ok"] * n
        col[k] = v
        AC.write_operands(str(workdir / "bad_ops.txt"), ([[b""] * n, col], []))
        assert AC.rejected(exe, cases, str(workdir / "bad_ops.txt"), two, []) == "args %d" % k, (k, v)


def test_sanitized_build_prints_the_same(workdir, corpus_out, directed_out):
    exe = str(workdir / "claims_match_args_test_asan")
    AC.build_host(exe, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for k, reqs in enumerate(AC.CORPUS_SETS):
        got = AC.run_host(exe, str(workdir / "cases.txt"), str(workdir / ("corpus_args%d.txt" % k)), reqs, env=env)
        assert got == corpus_out[reqs]
    for name, reqs in AC.PRED_SETS.items():
        got = AC.run_host(exe, str(workdir / "directed.txt"), str(workdir / "directed_args.txt"), reqs, env=env)
        assert got == directed_out[name]
