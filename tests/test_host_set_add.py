"""ClaimSet.Add without a GPU.

The host layer is built with g++ against a stand-in C ABI (tests/host_set_add/):

* set_add_stub.cpp: tests/host_match_set's stand-in plus jg_set_add, which is the
  CPU build of the insertion step the device runs
  (kernels/claim_set_insert.hpp), a switch that fails it, and a switch that
  loses the context.  The driver (set_add.cpp) checks that an Add is visible on
  the scan path and on the host path, the count it returns with repeats and
  resident members, that a failed add leaves both paths on the old members, the
  transition to host-only and Add on a host-only set, Add after Close, a NUL
  member, and that the added members are there after recover().
* the same driver linked with the stand-in built without jg_set_add: the same
  results come through a whole reload.
CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cap_amd", "csrc", "host")
HERE = os.path.join(ROOT, "tests", "host_set_add")


def build(exe, defines=()):
    assert shutil.which("g++"), "g++ is needed to build the host layer"
    srcs = [os.path.join(HERE, "set_add.cpp"), os.path.join(HERE, "set_add_stub.cpp")]
    srcs += [os.path.join(HOST, f) for f in ("hostmem.cpp", "json.cpp", "jose.cpp", "cap_jwt.cpp")]
    b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "tests", "host_kernels")] + list(defines) +
                       ["-o", exe] + srcs, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]


def test_add_against_the_stand_in_abi(tmp_path):
    exe = str(tmp_path / "set_add")
    build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "set add: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_a_library_without_jg_set_add_reloads_the_union(tmp_path):
    exe = str(tmp_path / "set_add_reload")
    build(exe, ["-DNO_SET_ADD"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "set add without jg_set_add: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_python_claim_set_has_add():
    J = pytest.importorskip("cap_amd.jwt")
    assert callable(J.ClaimSet.Add)
