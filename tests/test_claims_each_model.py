"""The per-profile claims scan (kernels/claims.hpp resolve_profiles and the
*_each functions) on the CPU: the code the k_claims_*_each kernels run, built as
a stand-alone program (tests/host_unit/claims_each_test.cpp).

* The corpus of tests/claims_corpus.py (5,970 cases over 190 Expected sets) runs
  in three tables of at most 64 profiles.  Codes, jg_claims and jg_selected are
  the single-Expect functions' -- claims_decide, claims_extract, claims_select
  as their own programs print them -- byte for byte.  Those are held to the
  oracle by their own tests.
* resolve_profiles() takes 64 profiles and exactly 8192 string bytes and refuses
  0 profiles, 65 profiles, 8193 bytes and a profile resolve() refuses.
* In a table filled to the last pool byte the last audience of profile 63
  matches and a value one byte longer does not.
* The program built under ASan + UBSan prints the same output.
CPU only; nothing is loaded into Python."""
import os

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_each_cases as EC
from tests import claims_extract_cases as XC
from tests import claims_select_cases as SC


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("claims_each")
    CC.write_cases(str(d / "cases.txt"))
    sets, cases, _ = EC.full_pool()
    EC.write_sets(str(d / "full.txt"), sets, cases)
    EC.build_host(str(d / "claims_each_test"))
    CC.build_host(str(d / "claims_scan_test"))
    XC.build_host(str(d / "claims_extract_test"))
    SC.build_host(str(d / "claims_select_test"))
    return d


@pytest.fixture(scope="module")
def single(workdir):
    """the single-Expect programs on the whole corpus: decide codes, (codes, records), (codes, records, selected)"""
    cases = str(workdir / "cases.txt")
    return (CC.run_host(str(workdir / "claims_scan_test"), cases),
            XC.run_host(str(workdir / "claims_extract_test"), cases),
            SC.run_host(str(workdir / "claims_select_test"), cases, EC.NAMES))


@pytest.fixture(scope="module")
def each_out(workdir):
    exe, cases = str(workdir / "claims_each_test"), str(workdir / "cases.txt")
    return {g: EC.run_host(exe, cases, g[0], g[1], EC.NAMES) for g in EC.groups()}


def test_corpus_shape():
    C = CC.corpus()
    assert len(C.all_cases()) == 5970 and len(C.sets) == 190
    assert EC.groups() == [(0, 64), (64, 128), (128, 190)]
    sizes = [sum(len(r[k]) for k in ("issuer", "subject", "id")) + sum(len(a) for a in r["audiences"])
             for r in (CC.resolve(*s) for s in C.sets)]
    # 1,271 characters; 1,277 bytes as UTF-8, which is what the pool holds
    assert sum(sizes) == 1277 and max(sizes) == 105


def test_each_equals_the_single_expect_functions(single, each_out):
    decide, (xcodes, xrecs), (scodes, srecs, ssels) = single
    seen = 0
    for (lo, hi), (d, (xc, xr), (sc, sr, sq)) in each_out.items():
        idx = EC.group_cases(lo, hi)
        assert len(d) == len(idx) > 0
        assert d == [decide[k] for k in idx], (lo, hi)
        assert xc == [xcodes[k] for k in idx] and xr == [xrecs[k] for k in idx], (lo, hi)
        assert sc == [scodes[k] for k in idx] and sr == [srecs[k] for k in idx], (lo, hi)
        assert sq == [ssels[k] for k in idx], (lo, hi)
        seen += len(idx)
    assert seen == 5970
    # every code occurs, and HOST records are zero
    allc = [c for d, _, _ in each_out.values() for c in d]
    assert set(allc) == set(range(_lib.CL_HOST + 1))
    for _, (xc, xr), (sc, sr, sq) in each_out.values():
        assert all(r == bytes(64) for c, r in zip(xc, xr) if c == _lib.CL_HOST)
        assert all(r == bytes(64) and q == bytes(80) for c, r, q in zip(sc, sr, sq) if c == _lib.CL_HOST)


def test_resolve_profiles_caps(workdir):
    exe = str(workdir / "claims_each_test")
    now = CC.T0 * CC.SECOND

    def table(name, sets):
        path = str(workdir / name)
        EC.write_sets(path, sets, [])
        return path
    full = table("cap_full.txt", EC.filler(64, 8192))
    assert not EC.rejected(exe, full, 0, 64)                                  # 64 profiles, exactly 8192 bytes
    assert EC.rejected(exe, full, 0, 0)                                       # no profile
    assert EC.rejected(exe, full, 5, 5)
    assert EC.rejected(exe, table("cap_over.txt", EC.filler(64, 8193)), 0, 64)    # one byte too many
    assert not EC.rejected(exe, table("cap_two.txt", EC.filler(2, 8192)), 0, 2)   # 4096 each: resolve()'s own cap
    assert EC.rejected(exe, table("cap_one.txt", EC.filler(1, 4097)), 0, 1)
    many = table("cap_65.txt", EC.filler(65, 650))
    assert EC.rejected(exe, many, 0, 65)                                      # 65 profiles
    assert not EC.rejected(exe, many, 1, 65) and not EC.rejected(exe, many, 0, 64)
    # one profile resolve() refuses among good ones: 17 audiences; now_nsec out of range
    good = EC.filler(3, 30)
    aud17 = CC.resolve({"Audiences": ["a%d" % k for k in range(17)]}, now)
    assert EC.rejected(exe, table("cap_aud17.txt", good[:2] + [aud17] + good[2:]), 0, 4)
    assert not EC.rejected(exe, table("cap_aud16.txt", good[:2] + [dict(aud17, audiences=aud17["audiences"][:16])]), 0, 3)
    assert EC.rejected(exe, table("cap_nsec.txt", good + [dict(good[0], now_nsec=10**9)]), 0, 4)
    assert not EC.rejected(exe, table("cap_nsec_ok.txt", good + [dict(good[0], now_nsec=10**9 - 1)]), 0, 4)


def test_full_pool_table(workdir):
    exe, path = str(workdir / "claims_each_test"), str(workdir / "full.txt")
    _, cases, want = EC.full_pool()
    d, (xc, _), (sc, _, _) = EC.run_host(exe, path, 0, 64, ("aud",))
    assert d == want and xc == want and sc == want
    # the same profiles one at a time through claims_decide
    CC.build_host(str(workdir / "claims_scan_test"))
    assert CC.run_host(str(workdir / "claims_scan_test"), path) == want


def test_sanitized_build_prints_the_same(workdir, each_out):
    exe = str(workdir / "claims_each_test_asan")
    EC.build_host(exe, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for g in EC.groups():
        assert EC.run_host(exe, str(workdir / "cases.txt"), g[0], g[1], EC.NAMES, env=env) == each_out[g]
    _, _, want = EC.full_pool()
    d, (xc, _), (sc, _, _) = EC.run_host(exe, str(workdir / "full.txt"), 0, 64, ("aud",), env=env)
    assert d == want and xc == want and sc == want
