"""The Validator::*Each entries (an Expected per token) without a GPU.  The host
layer is built with g++ against tests/host_each/each_stub.cpp, a stand-in C ABI
whose verify accepts every job and whose jg_claims_each runs the CPU build of the
device's functions (kernels/claims.hpp resolve_profiles and the *_each scans);
the driver (tests/host_each/each.cpp) runs a few hundred tokens of three tenants
whose profiles differ in issuer, audiences, Now and SigningAlgorithms -- with
wrong-tenant tokens, tokens expired for one profile only, payloads the scan
leaves to the host, a profile with 17 audiences (no device slot), 65 profiles in
use and a string pool that runs over -- and checks that CheckBatchEach,
CheckVerdictsEach, RegisteredBatchEach, RegisteredColsEach, SelectBatchEach and
SelectColsEach equal the existing entry called once per profile group and
scattered back (and ValidateBatch per group), that the stats sum up, that a
batch is one scan call, and the three std::invalid_argument cases.

A verifier library without jg_claims_each (the same stand-in built -DNO_EACH)
still links: every token that needed the scan gets a per-token "claims scan
unavailable" error, the profile without a slot is still answered by the host
path, and nothing crashes.  The driver is also built and run under ASan + UBSan
as a stand-alone program.  CPU only; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cap_amd", "csrc", "host")
HERE = os.path.join(ROOT, "tests", "host_each")
SOURCES = [os.path.join(HERE, "each.cpp")] + [
    os.path.join(HOST, f) for f in ("hostmem.cpp", "json.cpp", "jose.cpp", "cap_jwt.cpp")]


@pytest.fixture(scope="module")
def host_objects(tmp_path_factory):
    """the host layer and the driver, compiled once and linked with each stand-in"""
    assert shutil.which("g++"), "g++ is needed to build the host layer"
    d = tmp_path_factory.mktemp("host_each")
    objs = []
    for src in SOURCES:
        obj = str(d / (os.path.basename(src) + ".o"))
        b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-c", "-o", obj, src],
                           capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr[-3000:]
        objs.append(obj)
    return d, objs


def run_mode(host_objects, mode, defines=()):
    d, objs = host_objects
    exe = str(d / ("each_" + mode))
    b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-o", exe] + list(defines) + objs +
                       [os.path.join(HERE, "each_stub.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "each %s: ok" % mode in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_each_entries_equal_the_existing_ones_per_profile_group(host_objects):
    run_mode(host_objects, "ok")


def test_library_without_the_each_symbol(host_objects):
    run_mode(host_objects, "noeach", defines=["-DNO_EACH"])


def test_sanitized_stand_alone_build(tmp_path):
    exe = str(tmp_path / "each_asan")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe] + SOURCES +
                       [os.path.join(HERE, "each_stub.cpp")], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, "ok"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "each ok: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
