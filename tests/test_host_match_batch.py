"""The Match entries (Validator::MatchBatch, MatchVerdicts and the *Each forms)
without a GPU.  The host layer is built with g++ against
tests/host_match/match_stub.cpp, a stand-in C ABI whose verify accepts every job
and whose claims scans run the CPU build of the device's functions
(kernels/claims.hpp, claims_match_each included); the driver
(tests/host_match/match.cpp) checks the bits of device-decided rows (the scan's
masks), of JG_CL_HOST rows (match_requires on the verified claims map) and under
lists the ABI refuses (every token on the host path, stats.scanned == 0) against
match_requires on ValidateBatch's claims map and masks written by hand, ok / err
against CheckBatch, repeated requirements, MatchVerdicts against MatchBatch, the
*Each forms against one call per Expected, and what throws.

A verifier library without jg_claims_match (the same stand-in built -DNO_MATCH)
still links: every token that needed the scan gets a per-token "unavailable"
error, the other entries still work and nothing crashes.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cap_amd", "csrc", "host")
HERE = os.path.join(ROOT, "tests", "host_match")


@pytest.fixture(scope="module")
def host_objects(tmp_path_factory):
    """the host layer and the driver, compiled once and linked with each stand-in"""
    assert shutil.which("g++"), "g++ is needed to build the host layer"
    d = tmp_path_factory.mktemp("host_match")
    objs = []
    for src in [os.path.join(HERE, "match.cpp")] + [
            os.path.join(HOST, f) for f in ("hostmem.cpp", "json.cpp", "jose.cpp", "cap_jwt.cpp")]:
        obj = str(d / (os.path.basename(src) + ".o"))
        b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-c", "-o", obj, src],
                           capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr[-3000:]
        objs.append(obj)
    return d, objs


def run_mode(host_objects, mode, defines=()):
    d, objs = host_objects
    exe = str(d / ("match_" + mode))
    b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-o", exe] + list(defines) + objs
                       + [os.path.join(HERE, "match_stub.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "match %s: ok" % mode in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_bits_equal_the_evaluation_on_the_claims_map_on_both_paths_and_under_refused_lists(host_objects):
    run_mode(host_objects, "ok")


def test_library_without_the_match_symbol(host_objects):
    run_mode(host_objects, "nomatch", defines=["-DNO_MATCH"])
