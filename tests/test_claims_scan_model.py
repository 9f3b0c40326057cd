"""The registered-claims scan's decision function (kernels/claims.hpp) on the
CPU: the same code the GPU kernel runs, built as a stand-alone program
(tests/host_unit/claims_scan_test.cpp) and run on the corpus of
tests/claims_corpus.py.  Every code is HOST or exactly the string
oracle.jws.validate_claims gives; the plain list is decided without any HOST.
The program is built once more under ASan + UBSan and must agree with itself.
CPU only; nothing is loaded into Python."""
import os

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("claims_scan")
    CC.write_cases(str(d / "cases.txt"))
    return d


@pytest.fixture(scope="module")
def codes(workdir):
    exe = str(workdir / "claims_scan_test")
    CC.build_host(exe)
    return CC.run_host(exe, str(workdir / "cases.txt"))


def _slice(codes, which):
    C = CC.corpus()
    lo = {"plain": 0, "hard": len(C.plain), "random": len(C.plain) + len(C.hard)}[which]
    return lo, lo + len(getattr(C, which))


def test_corpus_covers_every_code_and_list():
    C = CC.corpus()
    want = CC.oracle_codes()
    assert len(C.plain) > 500 and len(C.hard) > 500 and len(C.random) >= 4000
    lo, hi = _slice(None, "plain")
    assert set(want[lo:hi]) == set(range(_lib.CL_HOST))          # each verdict occurs on the plain list
    assert None in want[hi:]                                      # payloads only the host may decide


def test_plain_list_is_decided_and_matches_the_oracle(codes):
    lo, hi = _slice(codes, "plain")
    want = CC.oracle_codes()
    C = CC.corpus()
    for k in range(lo, hi):
        seg, si = C.plain[k]
        assert codes[k] != _lib.CL_HOST, ("plain case left to the host", seg, C.sets[si])
        assert codes[k] == want[k], (codes[k], want[k], seg, C.sets[si])


def test_hard_and_random_lists_are_host_or_correct(codes):
    host = CC.check(codes)
    lo, hi = _slice(codes, "random")
    decided = sum(1 for c in codes[lo:hi] if c != _lib.CL_HOST)
    assert decided > 200, "the mutation pass must still reach the checks"
    assert host > 1000


def test_each_rule_has_a_case_the_scan_defers(codes):
    """One case per minimum rule that breaks only that rule: the scan says HOST
    (a scan that decided it could only be right by luck)."""
    C = CC.corpus()
    by_seg = {}
    for (seg, si), c in zip(C.all_cases(), codes):
        by_seg.setdefault(seg, set()).add(c)
    t = CC.T0 + 5
    only_host = [
        b'{"exp":1,"exp":%d}' % t,                         # a field named twice
        b'{"exp":%d,"EXP":1}' % t,                         # ... in another casing
        ('{"exp":%d,"ſub":"alice@example.com"}' % t).encode(),     # a byte >= 0x80 in a top-level key
        b'{"e\\u0078p":%d}' % (CC.T0 - 1000),              # an escape in a key
        b'{"exp":%d,"other":"a\\nb"}' % t,                 # an escape in another value
        b'{"exp":-0}', b'{"exp":1.5}', b'{"exp":1e999}', b'{"exp":1234567890123456}',
        b'{"exp":%d,"x":123456789012345678}' % t,          # a number of 18 bytes
        b'{"exp":%d,"x":1e3}' % t,                         # an exponent
        b"null", b"[1]", b"",
    ]
    for p in only_host:
        assert by_seg[CC.b64(p)] == {_lib.CL_HOST}, p


def test_sanitized_build_agrees(workdir, codes):
    exe = str(workdir / "claims_scan_test_asan")
    CC.build_host(exe, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    assert CC.run_host(exe, str(workdir / "cases.txt"), env=env) == codes
