"""The MatchArgs entries with hash columns (HashOfArg, IsString) without a GPU,
and match_requires with one token's hashed columns.

* The host layer is built with g++ against tests/host_match_hash/match_hash_stub.cpp,
  a stand-in C ABI whose verify accepts every job, whose jg_claims_match_hash runs
  the CPU build of the device's functions (kernels/claims.hpp and
  kernels/hash_operand.hpp) and whose jg_hash_batch hashes; the driver
  (tests/host_match_hash/match_hash.cpp) reads the tokens this test makes -- RS256,
  RS384, RS512 and EdDSA headers; at_hash right, wrong, absent, a number, null, "";
  a None entry; an access token of 8193 bytes; an escape in the payload; an expired
  token; no JWT at all -- with the mask the plain-Python evaluation owes, and checks
  bits, ok, stats, which ABI entry a call went to, the *Each and Verdicts forms,
  lists over the caps, a failed jg_hash_batch and what throws.
* match_requires with hashed columns (host/cap_jwt.cpp) against the plain-Python
  evaluation on the oracle's claims map over the directed list of
  tests/claims_match_hash_cases.py, the EdDSA / None entries (no value) included.
CPU only."""
import base64
import json
import os
import shutil
import subprocess

import pytest

from oracle import jws
from tests import claims_match_args_cases as AC
from tests import claims_match_hash_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cap_amd", "csrc", "host")
HERE = os.path.join(ROOT, "tests", "host_match_hash")
P = HC.P
T0 = 1611699344
REQS = (AC.EqA(P("nonce"), 0), HC.EqH(P("at_hash"), 0), HC.IsStr(P("at_hash")), HC.EqH(P("c_hash"), 1), HC.IsStr(P("c_hash")))
FAM = {"RS256": 1, "RS384": 2, "RS512": 3, "EdDSA": 0}


def b64(b):
    return base64.urlsafe_b64encode(b).rstrip(b"=").decode()


def token(alg, payload):
    sig = "A" * (86 if alg == "EdDSA" else 342)
    return b64(json.dumps({"alg": alg}, separators=(",", ":")).encode()) + "." + b64(payload) + "." + sig


def cases():
    """[(token, nonce, access token or None, code or None, ok, host, bits)]"""
    out = []
    tok, code = b"ya29.access-token", b"SplxlOBeZQQYbYS6WxSbIA"

    def add(alg, members, nonce=b"n-1", at=tok, cd=code, ok=True, host=False, exp=T0 + 600, raw=None):
        fam = FAM[alg]
        payload = raw if raw is not None else json.dumps(dict(members, nonce="n-1", exp=exp), separators=(",", ":")).encode()
        hs = [(at, fam) if at is not None and fam else None, (cd, fam) if cd is not None and fam else None]
        bits = HC.evaluate(jws._claims_map(payload), REQS, [nonce], [], hs)
        out.append((token(alg, payload), nonce, at, cd, ok, host, bits))
        return bits

    for alg in ("RS256", "RS384", "RS512"):
        fam = FAM[alg]
        right = {"at_hash": HC.hash_value(tok, fam).decode(), "c_hash": HC.hash_value(code, fam).decode()}
        assert add(alg, right) == 0b11111
        assert add(alg, right, at=b"another access token", nonce=b"n-2") == 0b11100
        assert add(alg, right, cd=AC.flip(code, 0)) == 0b10111
    r256 = {"at_hash": HC.hash_value(tok, 1).decode(), "c_hash": HC.hash_value(code, 1).decode()}
    assert add("RS384", r256) == 0b10101                                        # the family is the alg's, not the claim's
    assert add("RS256", {"c_hash": r256["c_hash"]}) == 0b11001                  # at_hash absent
    assert add("RS256", dict(r256, at_hash=7)) == 0b11001
    assert add("RS256", dict(r256, at_hash=None)) == 0b11001
    assert add("RS256", dict(r256, at_hash="")) == 0b11101
    assert add("EdDSA", r256) == 0b10101                                        # EdDSA: a string, never verified
    assert add("RS256", r256, at=None) == 0b11101                               # a None entry
    assert add("RS256", r256, at=None, cd=None) == 0b10101
    big = b"t" * 8193
    assert add("RS256", dict(r256, at_hash=HC.hash_value(big, 1).decode()), at=big, host=True) == 0b11111
    assert add("RS512", dict(r256, at_hash=HC.hash_value(b"t" * 8192, 3).decode()), at=b"t" * 8192) == 0b10111
    esc = (b'{"at_hash":"' + r256["at_hash"].encode() + b'","c_hash":"wrong","name":"a\\"b","nonce":"n-1","exp":%d}' % (T0 + 600))
    assert add("RS256", None, raw=esc, host=True) == 0b10111
    assert add("EdDSA", None, raw=esc, host=True) == 0b10101
    assert add("RS256", dict(r256), at=b"", cd=b"") == 0b10101                  # the empty value is a value
    assert add("RS256", {"at_hash": HC.hash_value(b"", 1).decode()}, at=b"") == 0b00111
    add("RS256", r256, ok=False, exp=T0 - 7200)                                 # expired: scanned, rejected
    out.append(("not-a-jwt", b"n-1", tok, code, False, False, 0))
    return out


def test_entries_against_the_stand_in_abi(tmp_path):
    assert shutil.which("g++"), "g++ is needed to build the host layer"
    exe = str(tmp_path / "match_hash")
    srcs = [os.path.join(HERE, "match_hash.cpp"), os.path.join(HERE, "match_hash_stub.cpp")] + [
        os.path.join(HOST, f) for f in ("hostmem.cpp", "json.cpp", "jose.cpp", "cap_jwt.cpp")]
    b = subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "tests", "host_kernels"), "-o", exe] + srcs,
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    hx = lambda v: "-" if v is None else "+" if not v else bytes(v).hex()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for tok, nonce, at, cd, ok, host, bits in cases():
            f.write("%s %s %s %s %d %d %d\n" % (tok, nonce.decode() or "-", hx(at), hx(cd), ok, host, bits))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "match hash: ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def native(reqs):
    out = []
    for path, op, value in reqs:
        if op <= AC.PRESENT:
            out.append((list(path), op, value, 0, 0))
        elif op in (AC.NUM_GE, AC.NUM_LE):
            out.append((list(path), op, "", value, 0))
        elif op == HC.IS_STRING:
            out.append((list(path), op, "", 0, 0))
        else:
            out.append((list(path), op, "", 0, value))
    return out


def test_match_requires_with_hashed_columns_on_the_directed_list():
    H = pytest.importorskip("cap_amd._capjwt_host")
    strs, nums, hashes = HC.directed_operands()
    n = none = hit = 0
    for name, reqs in HC.PRED_SETS.items():
        for k, payload in enumerate(HC.payloads()):
            s, hs = [col[k].decode() for col in strs], [col[k] for col in hashes]
            want = HC.evaluate(jws._claims_map(payload), reqs, [x.encode() for x in s], [], hs)
            hashed = [HC.hash_value(*h) if h is not None else None for h in hs]
            assert H.match_requires_hash(payload, native(reqs), s, [], hashed) == want, (payload, name, hs)
            n += 1
            none += any(h is None for h in hs)
            hit += any((want >> b) & 1 for b, r in enumerate(reqs) if r[1] == HC.EQUALS_HASH)
    assert n > 100 and none > 20 and hit > 20


def test_what_every_path_refuses():
    H = pytest.importorskip("cap_amd._capjwt_host")
    for reqs, hashed in (([(["a"], 10, "", 0, 1)], [b"x"]), ([(["a"], 10, "", 0, 0)], []), ([(["a"], 12, "", 0, 0)], [b"x"]),
                         ([(["a"], 11, "", 0, 0)] * 17, [])):
        with pytest.raises(ValueError):
            H.match_requires_hash(b"{}", reqs, [], [], hashed)
    assert H.match_requires_hash(b'{"a":"s","b":1}', [(["a"], 11, "", 0, 0), (["b"], 11, "", 0, 0), (["a"], 10, "", 0, 0),
                                                      (["a"], 10, "", 0, 1)], [], [], [b"s", None]) == 0b0101
    # the entries without hash columns keep refusing the new ops
    for op in (10, 11):
        with pytest.raises(ValueError):
            H.match_requires(b"{}", [(["a"], op, "")])
        with pytest.raises(ValueError):
            H.match_requires_args(b"{}", [(["a"], op, "", 0, 0)], ["x"], [])
