"""The Select entries by path (Validator::SelectBatch and kin with ClaimPaths)
without a GPU.  The host layer is built with g++ against
tests/host_paths/paths_stub.cpp, a stand-in C ABI whose verify accepts every job
and whose claims scans run the CPU build of the device's functions
(kernels/claims.hpp, claims_paths_each included); the driver
(tests/host_paths/paths.cpp) checks the values of device-decided rows (from the
jg_selected records), of JG_CL_HOST rows (from the verified claims map) and
under path lists the ABI refuses (every token on the host path,
stats.scanned == 0) against the walk of ValidateBatch's claims map, ok / err
against CheckBatch, one-component paths against the names, the *Each form against
one call per Expected, and SelectCols against SelectBatch.

A verifier library without jg_claims_paths (the same stand-in built -DNO_PATHS)
still links: every token that needed the scan gets a per-token "unavailable"
error, the entries by name still work and nothing crashes.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cap_amd", "csrc", "host")
HERE = os.path.join(ROOT, "tests", "host_paths")


@pytest.fixture(scope="module")
def host_objects(tmp_path_factory):
    """the host layer and the driver, compiled once and linked with each stand-in"""
    assert shutil.which("g++"), "g++ is needed to build the host layer"
    d = tmp_path_factory.mktemp("host_paths")
    objs = []
    for src in [os.path.join(HERE, "paths.cpp")] + [
            os.path.join(HOST, f) for f in ("hostmem.cpp", "json.cpp", "jose.cpp", "cap_jwt.cpp")]:
        obj = str(d / (os.path.basename(src) + ".o"))
        b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-c", "-o", obj, src],
                           capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr[-3000:]
        objs.append(obj)
    return d, objs


def run_mode(host_objects, mode, defines=()):
    d, objs = host_objects
    exe = str(d / ("paths_" + mode))
    b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-o", exe] + list(defines) + objs
                       + [os.path.join(HERE, "paths_stub.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "paths %s: ok" % mode in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_values_equal_the_claims_map_walk_on_both_paths_and_under_refused_lists(host_objects):
    run_mode(host_objects, "ok")


def test_library_without_the_paths_symbol(host_objects):
    run_mode(host_objects, "nopaths", defines=["-DNO_PATHS"])
