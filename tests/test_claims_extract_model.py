"""The extracting claims scan (kernels/claims.hpp claims_extract) on the CPU: the
code k_claims_extract runs, built as a stand-alone program
(tests/host_unit/claims_extract_test.cpp) and run on the corpus of
tests/claims_corpus.py plus the directed list of tests/claims_extract_cases.py.

* The codes are claims_decide's (the claims_scan_test program's), case for case.
* Every non-HOST record, cut out of the decoded payload, is the oracle's
  jwt.Claims (oracle.jws._claims_struct); every HOST record is 64 zero bytes;
  nothing on the plain list or the directed list is HOST.
* The program built under ASan + UBSan prints the same output.
CPU only; nothing is loaded into Python."""
import os

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("claims_extract")
    CC.write_cases(str(d / "cases.txt"))
    XC.write_cases(str(d / "directed.txt"), XC.directed())
    XC.build_host(str(d / "claims_extract_test"))
    return d


@pytest.fixture(scope="module")
def corpus_out(workdir):
    return XC.run_host(str(workdir / "claims_extract_test"), str(workdir / "cases.txt"))


@pytest.fixture(scope="module")
def directed_out(workdir):
    return XC.run_host(str(workdir / "claims_extract_test"), str(workdir / "directed.txt"))


@pytest.fixture(scope="module")
def decide_exe(workdir):
    exe = str(workdir / "claims_scan_test")
    CC.build_host(exe)
    return exe


def test_codes_equal_claims_decide(workdir, corpus_out, directed_out, decide_exe):
    assert corpus_out[0] == CC.run_host(decide_exe, str(workdir / "cases.txt"))
    assert directed_out[0] == CC.run_host(decide_exe, str(workdir / "directed.txt"))


def test_corpus_records_are_the_oracles_claims(corpus_out):
    codes, recs = corpus_out
    C = CC.corpus()
    cases = XC.corpus_cases()
    CC.check(codes)                                          # HOST or the oracle's string; the plain list decided
    nplain = len(C.plain)
    assert XC.check_records(cases[:nplain], codes[:nplain], recs[:nplain], no_host=True) == nplain
    decided = XC.check_records(cases[nplain:], codes[nplain:], recs[nplain:])
    assert decided > 200                                     # hard and random cases still reach the record
    assert sum(1 for c in codes if c == _lib.CL_HOST) > 1000
    failing = {c for c in codes if c not in (_lib.CL_OK, _lib.CL_HOST)}
    assert failing == set(range(1, _lib.CL_HOST))            # a failure code carries a filled record too


def test_directed_list(directed_out):
    codes, recs = directed_out
    cases = XC.directed()
    assert len(cases) > 5040
    assert XC.check_records(cases, codes, recs, no_host=True) == len(cases)
    by_payload = {XC.payload_of(seg): XC.unpack(r) for (seg, _, _), r in zip(cases, recs)}
    t = CC.T0
    # "" against null: the bit, and the position after the opening quote
    v = by_payload[b'{"sub":"","iat":%d}' % t]
    assert (v["present"] >> _lib.F_SUB) & 1 and (v["sub_off"], v["sub_len"]) == (8, 0)
    v = by_payload[b'{"sub":null,"iat":%d}' % t]
    assert not (v["present"] >> _lib.F_SUB) & 1 and (v["sub_off"], v["sub_len"]) == (0, 0)
    # exp = 0 present against exp absent
    assert (by_payload[b'{"exp":0,"iat":%d}' % t]["present"] >> _lib.F_EXP) & 1
    assert not (by_payload[b'{"iat":%d}' % t]["present"] >> _lib.F_EXP) & 1
    # aud: the value's text and its element count
    v = by_payload[b'{"aud":[],"exp":%d}' % (t + 5)]
    assert (v["aud_off"], v["aud_len"], v["aud_n"]) == (7, 2, 0) and (v["present"] >> _lib.F_AUD) & 1
    v = by_payload[b'{"aud":"solo","exp":%d}' % (t + 5)]
    assert (v["aud_off"], v["aud_len"], v["aud_n"]) == (7, 6, 1)
    assert max(XC.unpack(r)["aud_n"] for r in recs) == 16
    assert {XC.unpack(r)["sub_off"] % 3 for r in recs} == {0, 1, 2}


def test_sanitized_build_prints_the_same(workdir, corpus_out, directed_out):
    exe = str(workdir / "claims_extract_test_asan")
    XC.build_host(exe, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    assert XC.run_host(exe, str(workdir / "cases.txt"), env=env) == corpus_out
    assert XC.run_host(exe, str(workdir / "directed.txt"), env=env) == directed_out
