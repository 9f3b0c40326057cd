"""Validator::RegisteredBatch's host merge without a GPU.  The host layer is
built with g++ against tests/host_registered/accept_stub.cpp, a stand-in C ABI
whose verify accepts every job and whose claims scans run the CPU build of the
device's decision functions (kernels/claims.hpp); the driver
(tests/host_registered/registered.cpp) checks the claims of device-decided rows
(from the records), of JG_CL_HOST rows (from the struct validate_claims
decodes) and both aud forms against values written into it, and ok / err
against CheckBatch.

A verifier library without jg_claims_extract (the same stand-in built
-DNO_EXTRACT, and tests/host_faults/fault_stub.cpp, whose device calls all
fail) still links: every token that needed the scan gets a per-token
"unavailable" error and nothing crashes.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cap_amd", "csrc", "host")
HERE = os.path.join(ROOT, "tests", "host_registered")
FAULTS = os.path.join(ROOT, "tests", "host_faults")


@pytest.fixture(scope="module")
def host_objects(tmp_path_factory):
    """the host layer and the driver, compiled once and linked with each stand-in"""
    assert shutil.which("g++"), "g++ is needed to build the host layer"
    d = tmp_path_factory.mktemp("host_registered")
    objs = []
    for src in [os.path.join(HERE, "registered.cpp")] + [
            os.path.join(HOST, f) for f in ("hostmem.cpp", "json.cpp", "jose.cpp", "cap_jwt.cpp")]:
        obj = str(d / (os.path.basename(src) + ".o"))
        b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-c", "-o", obj, src],
                           capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr[-3000:]
        objs.append(obj)
    return d, objs


def run_mode(host_objects, mode, stub, defines=()):
    d, objs = host_objects
    exe = str(d / ("registered_" + mode))
    b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-o", exe] + list(defines) + objs + [stub],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "registered %s: ok" % mode in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_claims_from_records_and_from_the_host_struct(host_objects):
    run_mode(host_objects, "ok", os.path.join(HERE, "accept_stub.cpp"))


def test_library_without_the_extract_symbol(host_objects):
    run_mode(host_objects, "noextract", os.path.join(HERE, "accept_stub.cpp"), defines=["-DNO_EXTRACT"])


def test_fault_stub_still_links_and_gives_per_token_errors(host_objects):
    run_mode(host_objects, "fault", os.path.join(FAULTS, "fault_stub.cpp"))
