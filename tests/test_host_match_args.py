"""The MatchArgs entries (Validator::MatchBatchArgs, MatchVerdictsArgs and the
*Each forms) without a GPU, and match_requires with one token's operands.

* The host layer is built with g++ against tests/host_match_args/match_args_stub.cpp,
  a stand-in C ABI whose verify accepts every job and whose claims scans run the
  CPU build of the device's functions (kernels/claims.hpp, claims_match_args
  included); the driver (tests/host_match_args/match_args.cpp) checks the bits of
  device-decided rows and of host-path rows against match_requires on
  ValidateBatch's claims map and masks written by hand, ok / err against
  CheckBatch, that a token with an operand the scan refuses takes the host path
  and no refused operand reaches the ABI, lists over the caps, MatchVerdictsArgs
  against MatchBatchArgs, the *Each forms against one call per Expected, what
  throws, and that the MatchBatch family still refuses the new ops.
* match_requires with operands (host/cap_jwt.cpp) against the plain-Python
  evaluation on the oracle's claims map: every predicate set of
  tests/claims_match_args_cases.py on every directed payload with its operands
  -- fractions, 16 and 17 digits and bytes >= 0x80 among them, the cases only the
  host decides -- and some the scan would not take.
CPU only."""
import os
import shutil
import subprocess

import pytest

from oracle import jws
from tests import claims_match_args_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cap_amd", "csrc", "host")
HERE = os.path.join(ROOT, "tests", "host_match_args")
P = AC.P


def test_entries_against_the_stand_in_abi(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host layer"
    exe = str(tmp_path / "match_args")
    srcs = [os.path.join(HERE, "match_args.cpp"), os.path.join(HERE, "match_args_stub.cpp")] + [
        os.path.join(HOST, f) for f in ("hostmem.cpp", "json.cpp", "jose.cpp", "cap_jwt.cpp")]
    b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-o", exe] + srcs, capture_output=True, text=True,
                       timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "match args: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def native(reqs):
    out = []
    for path, op, value in reqs:
        if op <= AC.PRESENT:
            out.append((list(path), op, value, 0, 0))
        elif op in (AC.NUM_GE, AC.NUM_LE):
            out.append((list(path), op, "", value, 0))
        else:
            out.append((list(path), op, "", 0, value))
    return out


def test_match_requires_with_operands_on_the_directed_list():
    H = pytest.importorskip("cap_amd._capjwt_host")
    strs, nums = AC.directed_operands()
    n = hosts = 0
    for name, reqs in AC.PRED_SETS.items():
        for k, payload in enumerate(AC.payloads()):
            s, v = [col[k].decode() for col in strs], [col[k] for col in nums]
            want = AC.evaluate(jws._claims_map(payload), reqs, [x.encode() for x in s], v)
            assert H.match_requires_args(payload, native(reqs), s, v) == want, (payload, name, s, v)
            n += 1
            hosts += k in AC.directed_hosts(name)
    assert n > 500 and hosts > 20                       # the fractions and long numbers are among them


def test_match_requires_with_operands_the_scan_does_not_take():
    H = pytest.importorskip("cap_amd._capjwt_host")
    payload = ('{"nonce":"nønce \\"q\\"","auth_time":1611699344.25,"big":12345678901234567,"neg":-0.5,'
               '"e":1e3,"long":"' + "v" * 70 + '","deep":{"a":{"b":{"c":{"d":{"n":2}}}}},"t":true}').encode()
    strs = ['nønce "q"', "v" * 70, "nonce"]
    nums = [1611699344, 1611699345, 12345678901234568, AC.INT64_MIN]
    reqs = (AC.EqA(P("nonce"), 0), AC.EqA(P("long"), 1), AC.EqA(P("nonce"), 2), AC.GeA(P("auth_time"), 0),
            AC.LeA(P("auth_time"), 0), AC.LeA(P("auth_time"), 1), AC.GeA(P("big"), 2), AC.LeA(P("big"), 2),
            AC.Ge(P("neg"), 0), AC.Le(P("neg"), 0), AC.Ge(P("e"), 1000), AC.Ge(P("deep", "a", "b", "c", "d", "n"), 2),
            AC.GeA(P("neg"), 3), AC.Ge(P("t"), 0), AC.Le(P("big"), AC.INT64_MAX), AC.Ge(P("long"), 0))
    assert len(reqs) == 16
    want = AC.evaluate(jws._claims_map(payload), reqs, [x.encode() for x in strs], nums)
    # 12345678901234567 and ...68 are one float64, so both compares with it hold
    assert H.match_requires_args(payload, native(reqs), strs, nums) == want == 0b0101_1110_1110_1011


def test_what_every_path_refuses():
    H = pytest.importorskip("cap_amd._capjwt_host")
    for reqs, strs, nums in (([(["a"], 6, "", k, 0) for k in range(17)], [], []), ([([], 6, "", 0, 0)], [], []),
                             ([(["a"], 10, "", 0, 0)], [], []), ([(["a"], 0, "", 0, 0)], [], []),
                             ([(["a"], 5, "", 0, 1)], ["x"], []), ([(["a"], 8, "", 0, 0)], ["x"], []),
                             ([(["a"], 9, "", 0, 2)], [], [1, 2]), ([(["a", "b\0"], 6, "", 0, 0)], [], [])):
        with pytest.raises(ValueError):
            H.match_requires_args(b"{}", reqs, strs, nums)
    assert H.match_requires_args(b'{"a":1}', [], [], []) == 0
    # the entry without operands keeps refusing the new ops
    for op in (5, 6, 7, 8, 9):
        with pytest.raises(ValueError):
            H.match_requires(b"{}", [(["a"], op, "")])
