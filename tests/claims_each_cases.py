"""Shared by the tests of the per-profile claims scan (jg_claims_each): the
corpus of tests/claims_corpus.py cut into groups of at most JG_MAX_PROFILES
Expected sets, a table filled to the last byte of its string pool, and the host
program tests/host_unit/claims_each_test.cpp."""
import os
import shutil
import subprocess

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_select_cases as SC

ROOT = CC.ROOT
T0 = CC.T0
NAMES = SC.CORPUS_NAMES                      # the select names of the corpus runs


def groups():
    """[lo, hi) ranges over the corpus's Expected sets, at most JG_MAX_PROFILES each"""
    n = len(CC.corpus().sets)
    return [(lo, min(lo + _lib.MAX_PROFILES, n)) for lo in range(0, n, _lib.MAX_PROFILES)]


def group_cases(lo, hi):
    """indices into corpus().all_cases() of the cases whose set lies in [lo, hi)"""
    return [k for k, (_, si) in enumerate(CC.corpus().all_cases()) if lo <= si < hi]


def write_sets(path, sets, cases):
    """sets: resolved dicts (claims_corpus.resolve), in order and kept apart even
    when equal; cases: (set index, segment)"""
    with open(path, "w") as f:
        for r in sets:
            f.write("E %s %s %s %d %s%d %d %d %d %d\n" % (
                CC._hex(r["issuer"]), CC._hex(r["subject"]), CC._hex(r["id"]), len(r["audiences"]),
                "".join(CC._hex(a) + " " for a in r["audiences"]), r["now_sec"], r["now_nsec"], r["skew_ns"],
                r["exp_leeway_s"], r["nbf_leeway_s"]))
        for si, seg in cases:
            f.write("C %d %s\n" % (si, CC._hex(seg)))


def filler(nprofiles, total):
    """nprofiles resolved sets whose strings are `total` bytes in all: issuers only"""
    now = T0 * CC.SECOND
    each, extra = divmod(total, nprofiles)
    out = []
    for p in range(nprofiles):
        ln = each + (1 if p < extra else 0)
        out.append(CC.resolve({"Issuer": ("p%02d-" % p + "i" * ln)[:ln]}, now))
    return out


def full_pool():
    """-> (sets, cases, want): JG_MAX_PROFILES resolved sets whose strings fill the
    pool to its last byte (63 x 128 bytes of issuer; profile 63: 64 of issuer and
    two audiences of 32, the second ending at byte JG_PROFILE_POOL_BYTES - 1), the
    cases (set index, segment) and the code each must get."""
    assert _lib.MAX_PROFILES == 64 and _lib.PROFILE_POOL_BYTES == 8192
    sets = filler(63, 63 * 128)
    iss = "https://last.example/" + "i" * 43
    a0, a1 = "first-" + "a" * 26, "last--" + "z" * 26
    assert len(iss) == 64 and len(a0) == 32 and len(a1) == 32
    sets.append(CC.resolve({"Issuer": iss, "Audiences": [a0, a1]}, T0 * CC.SECOND))
    assert sum(len(r["issuer"]) + sum(len(a) for a in r["audiences"]) for r in sets) == _lib.PROFILE_POOL_BYTES
    pay = lambda i, a: CC.b64(CC.js({"iss": i, "aud": a, "exp": T0 + 100}))   # nbf defaults to exp - 150 s
    cases = [
        (63, pay(iss, a1), _lib.CL_OK),                    # the pool's last 32 bytes
        (63, pay(iss, [a0 + "x", a1]), _lib.CL_OK),
        (63, pay(iss, a1 + "z"), _lib.CL_AUD),             # one byte longer: past the pool's end
        (63, pay(iss, a1[:-1]), _lib.CL_AUD),
        (63, pay(iss, a0), _lib.CL_OK),
        (63, pay(iss + "i", a1), _lib.CL_ISS),
        (62, pay(sets[62]["issuer"].decode(), "x"), _lib.CL_OK),
        (62, pay(sets[62]["issuer"].decode() + "h", "x"), _lib.CL_ISS),   # the next pool byte is profile 63's 'h'
        (0, pay(sets[0]["issuer"].decode(), "x"), _lib.CL_OK),
        (0, pay(sets[1]["issuer"].decode(), "x"), _lib.CL_ISS),
    ]
    return sets, [(si, seg) for si, seg, _ in cases], [w for _, _, w in cases]


def build_host(exe, sanitize=False):
    """Compile tests/host_unit/claims_each_test.cpp (the *_each functions for the CPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the scan's host model"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host_unit", "claims_each_test.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


def run_host(exe, cases_path, lo, hi, names=(), env=None):
    """-> (decide codes, (extract codes, records), (select codes, records, selected))"""
    r = subprocess.run([exe, cases_path, str(lo), str(hi)] + SC.name_args(names), capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    d, xc, xr, sc, sr, sq = [], [], [], [], [], []
    for line in r.stdout.splitlines():
        a, b, c, e, f, g = line.split()
        d.append(int(a))
        xc.append(int(b))
        xr.append(bytes.fromhex(c))
        sc.append(int(e))
        sr.append(bytes.fromhex(f))
        sq.append(bytes.fromhex(g))
    return d, (xc, xr), (sc, sr, sq)


def rejected(exe, cases_path, lo, hi, names=()):
    """True when resolve_profiles() (or resolve_select()) refuses"""
    r = subprocess.run([exe, cases_path, str(lo), str(hi)] + SC.name_args(names), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode in (0, 3), (r.returncode, r.stderr[-2000:])
    assert (r.returncode == 3) == (r.stdout.strip() == "rejected")
    return r.returncode == 3
