"""The resolvers of kernels/claims.hpp -- resolve(), resolve_profiles(),
resolve_select() and resolve_paths() -- on the CPU: the stand-alone program
tests/host_unit/claims_resolve_test.cpp runs them on a fixed list of inputs and
prints the bytes each one fills.

* The SHA-256 of every filled object is the one recorded in
  tests/golden/claims_resolve_digests.txt.  These bytes are what the claims
  kernels copy to LDS and read, so the device sees the same expected side, names
  and paths as when the file was recorded (from the commit before resolve() and
  resolve_profiles() came to share their per-profile part).
* The inputs each resolver refuses are the ones listed here, and no other.
* The program built under ASan + UBSan prints the same output.
CPU only; nothing is loaded into Python."""
import hashlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "claims_resolve_digests.txt")

# sizeof(Expect), sizeof(Profiles), sizeof(Select), sizeof(Paths)
SIZES = {"resolve": 4216, "resolve_profiles": 8 + 120 * 64 + 8192, "resolve_select": 548, "resolve_paths": 2172}

REFUSED = {
    "resolve": {"over_max_bytes", "over_max_bytes_in_auds", "nsec_1e9", "null_strs", "seventeen_auds"},
    "resolve_profiles": {"one_over_max_bytes", "one_over_max_bytes_in_auds", "one_nsec_1e9", "one_null_strs",
                         "one_seventeen_auds", "sixty_five", "pool_over_by_one", "pool_full_then_one_byte", "none",
                         "second_over_max_bytes", "second_nsec_1e9", "null_strs", "null_expects"},
    "resolve_select": {"nine", "empty_name", "65_bytes", "byte_1f", "byte_7f", "byte_80", "byte_00", "quote",
                       "backslash", "equal_names", "equal_names_of_64", "null_names"},
    "resolve_paths": {"nine", "no_component", "five_components", "empty_component", "empty_first_component",
                      "65_bytes", "byte_1f", "byte_7f", "byte_80", "byte_00", "quote", "backslash", "equal_paths",
                      "equal_paths_of_4", "null_names"},
}

# the inputs at the limits, which must be on the list and must resolve
AT_THE_LIMITS = ["resolve/all_empty", "resolve/sixteen_empty_auds", "resolve/sixteen_auds", "resolve/max_bytes_one_string",
                 "resolve/max_bytes_last_aud", "resolve/negative_now_largest_skew", "resolve_profiles/sixty_four",
                 "resolve_profiles/pool_full_sixty_four", "resolve_profiles/pool_full_two",
                 "resolve_profiles/one_max_bytes_one_string", "resolve_select/eight_of_64",
                 "resolve_paths/eight_of_4_of_64", "resolve_paths/eight_of_4"]


def build_host(exe, sanitize=False):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the resolvers' host program"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host_unit", "claims_resolve_test.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


def run_host(exe, env=None):
    """-> {"resolver/case": "refused" or the SHA-256 of the filled bytes}, in the program's order"""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    out = {}
    for line in r.stdout.splitlines():
        name, val = line.split(" ")
        assert name not in out, name
        if val != "refused":
            raw = bytes.fromhex(val)
            assert len(raw) == SIZES[name.split("/")[0]], name
            val = hashlib.sha256(raw).hexdigest()
        out[name] = val
    return out


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("claims_resolve")
    build_host(str(d / "claims_resolve_test"))
    return d


@pytest.fixture(scope="module")
def digests(workdir):
    return run_host(str(workdir / "claims_resolve_test"))


def golden():
    with open(GOLDEN) as f:
        return dict(line.split() for line in f if line.strip() and not line.startswith("#"))


def test_resolved_bytes_are_the_recorded_ones(digests):
    want = golden()
    assert list(digests) == list(want)
    for name, val in digests.items():
        assert val == want[name], name


def test_refused_inputs_are_the_listed_ones(digests):
    for resolver, names in REFUSED.items():
        got = {n.split("/")[1] for n, v in digests.items() if n.startswith(resolver + "/") and v == "refused"}
        assert got == names, resolver
    for name in AT_THE_LIMITS:
        assert digests[name] != "refused", name


def test_sanitized_build_prints_the_same(workdir, digests):
    exe = str(workdir / "claims_resolve_test_asan")
    build_host(exe, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    assert run_host(exe, env=env) == digests
