"""Validator::SelectBatch's host merge without a GPU.  The host layer is built
with g++ against tests/host_select/select_stub.cpp, a stand-in C ABI whose
verify accepts every job and whose claims scans run the CPU build of the
device's functions (kernels/claims.hpp, claims_select included); the driver
(tests/host_select/select.cpp) checks the values of device-decided rows (from
the jg_selected records), of JG_CL_HOST rows (from the verified claims map) and
under a name list the ABI refuses (every token on the host path,
stats.scanned == 0) against ValidateBatch's map entries, ok / err against
CheckBatch, the claims against RegisteredBatch, and SelectCols against
SelectBatch -- an array's text being json::marshal's on both paths.

A verifier library without jg_claims_select (the same stand-in built
-DNO_SELECT, and tests/host_faults/fault_stub.cpp, whose device calls all
fail) still links: every token that needed the scan gets a per-token
"unavailable" error and nothing crashes.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cap_amd", "csrc", "host")
HERE = os.path.join(ROOT, "tests", "host_select")
FAULTS = os.path.join(ROOT, "tests", "host_faults")


@pytest.fixture(scope="module")
def host_objects(tmp_path_factory):
    """the host layer and the driver, compiled once and linked with each stand-in"""
    assert shutil.which("g++"), "g++ is needed to build the host layer"
    d = tmp_path_factory.mktemp("host_select")
    objs = []
    for src in [os.path.join(HERE, "select.cpp")] + [
            os.path.join(HOST, f) for f in ("hostmem.cpp", "json.cpp", "jose.cpp", "cap_jwt.cpp")]:
        obj = str(d / (os.path.basename(src) + ".o"))
        b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-c", "-o", obj, src],
                           capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr[-3000:]
        objs.append(obj)
    return d, objs


def run_mode(host_objects, mode, stub, defines=()):
    d, objs = host_objects
    exe = str(d / ("select_" + mode))
    b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-o", exe] + list(defines) + objs + [stub],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "select %s: ok" % mode in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_values_from_records_from_the_map_and_under_a_refused_name_list(host_objects):
    run_mode(host_objects, "ok", os.path.join(HERE, "select_stub.cpp"))


def test_library_without_the_select_symbol(host_objects):
    run_mode(host_objects, "noselect", os.path.join(HERE, "select_stub.cpp"), defines=["-DNO_SELECT"])


def test_fault_stub_still_links_and_gives_per_token_errors(host_objects):
    run_mode(host_objects, "fault", os.path.join(FAULTS, "fault_stub.cpp"))
