"""The MatchArgs entries with InSet / AnyElementIn and ClaimSet without a GPU.

The host layer is built with g++ against a stand-in C ABI and a driver that
makes its own tokens (tests/host_match_set/):

* match_set_stub.cpp: verify accepts every job; jg_set_load / jg_set_free /
  jg_set_info keep sets built by set_build(); jg_claims_match_set runs the CPU
  build of the device's scan (kernels/claims.hpp claims_match_set).  The driver
  checks both paths (the scan's tokens and the host path's, an escape in a
  payload), a host-only set for every kind of member the device refuses, four
  sets scanned and five answered from the host path with the same bits, Replace
  and Close under the failure policy, the 17th live set, the seed, and what
  throws.
* the same driver as `nolib`, linked with the stand-in of the hash entries
  alone: a library without jg_set_* and jg_claims_match_set still links, and a
  call that names a set reports the scan as unavailable per token.
CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cap_amd", "csrc", "host")
HERE = os.path.join(ROOT, "tests", "host_match_set")


def build(exe, stub):
    assert shutil.which("g++"), "g++ is needed to build the host layer"
    srcs = [os.path.join(HERE, "match_set.cpp"), stub] + [os.path.join(HOST, f) for f in ("hostmem.cpp", "json.cpp", "jose.cpp", "cap_jwt.cpp")]
    b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "tests", "host_kernels"), "-o", exe] + srcs,
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]


def test_entries_against_the_stand_in_abi(tmp_path):
    exe = str(tmp_path / "match_set")
    build(exe, os.path.join(HERE, "match_set_stub.cpp"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "match set: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_a_library_without_the_set_entries_still_links(tmp_path):
    exe = str(tmp_path / "match_set_nolib")
    build(exe, os.path.join(ROOT, "tests", "host_match_hash", "match_hash_stub.cpp"))
    r = subprocess.run([exe, "nolib"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "match set nolib: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_python_requirements():
    J = pytest.importorskip("cap_amd.jwt")
    with pytest.raises(TypeError):
        J.InSet("jti", ["not", "a", "ClaimSet"])
    with pytest.raises(TypeError):
        J.AnyElementIn(J.Path("a", "b"), None)
    assert J.SetRequire.IN_SET == 12 and J.SetRequire.ELEMENT_IN_SET == 13
    assert {"ClaimSet", "InSet", "AnyElementIn"} <= set(J.__all__)
