"""Shared by the tests of the extracting claims scan (claims_extract /
k_claims_extract / jg_claims_extract): the directed case list, the host build of
tests/host_unit/claims_extract_test.cpp, and the check of a jg_claims record
against the oracle's jwt.Claims (oracle.jws._claims_struct).

The corpus itself is tests/claims_corpus.py's; the directed list adds what it
may not pin: field order, "" and null, the aud forms, a sub at every decoded
offset mod 3, exp = 0 against exp absent, 15-digit and negative dates, key
casing.
"""
import base64
import functools
import itertools
import os
import shutil
import struct
import subprocess

from cap_amd import _lib
from oracle import jws
from tests import claims_corpus as CC

ROOT = CC.ROOT
T0 = CC.T0
RECORD = struct.Struct("<qqq10I")            # jg_claims (include/jg.h)
FIELDS = ("exp", "nbf", "iat", "iss_off", "iss_len", "sub_off", "sub_len", "jti_off", "jti_len",
          "aud_off", "aud_len", "aud_n", "present")
assert RECORD.size == 64


@functools.lru_cache(maxsize=1)
def directed():
    """[(segment, expected dict, now_ns)]; every case follows the scan's rules
    (decided, never HOST)."""
    out = []
    now = T0 * CC.SECOND

    def add(payload, expected=None):
        out.append((CC.b64(payload), expected or {}, now))

    members = [b'"iss":"https://example.com/"', b'"sub":"alice@example.com"', b'"jti":"std"',
               b'"aud":["www.example.com","b"]', b'"exp":%d' % (T0 + 600), b'"nbf":%d' % T0, b'"iat":%d' % (T0 - 1)]
    for order in itertools.permutations(range(7)):                 # registered fields in every order
        add(b"{" + b",".join(members[k] for k in order) + b"}", CC.FULL)
    for key in (b"iss", b"sub", b"jti"):                           # "" and null
        for v in (b'""', b"null"):
            for lead in (b"", b'"exp":%d,' % (T0 + 5)):
                add(b"{" + lead + b'"' + key + b'":' + v + b',"iat":%d}' % T0)
                add(b"{" + lead + b'"' + key + b'":' + v + b',"iat":%d}' % T0, CC.FULL)
    for key in (b"exp", b"nbf", b"iat"):
        add(b'{"' + key + b'":null,"x":1,"' + (b"iat" if key != b"iat" else b"exp") + b'":%d}' % T0)
    add(b'{"iss":null,"sub":null,"jti":null,"exp":null,"nbf":null,"iat":null}')
    add(b'{"iss":"","sub":"","jti":"","aud":"","exp":%d}' % (T0 + 5))
    sixteen = b'[ "a00" ,\t"a01",\n"a02",\r"a03", "a04","a05" , "a06","","a08","a09","a10","a11","a12","a13","a14" , "a15" ]'
    for aud in (b'"solo"', b"[]", b'["one"]', b'["one","two"]', b'[ ]', b'[ "one" ]', b'""', b'[""]', sixteen):
        for ex in ({}, {"Audiences": ["a15", "two"]}):
            add(b'{"aud":' + aud + b',"exp":%d}' % (T0 + 5), ex)
            add(b'{"exp":%d, "aud" : ' % (T0 + 5) + aud + b' }', ex)
            add(b'{"exp":%d,"aud":' % (T0 + 5) + aud + b',"sub":"after"}', ex)
    for shift in range(3):                                         # a sub at every decoded offset mod 3
        for ln in range(6):
            add(b'{"p":"' + b"x" * shift + b'","sub":"' + b"abcde"[:ln] + b'","exp":%d}' % (T0 + 5))
            add(b'{"exp":%d,"p":"' % (T0 + 5) + b"x" * shift + b'","sub":"' + b"abcde"[:ln] + b'"}')   # ends the text
    add(b'{"exp":0,"iat":%d}' % T0)                                # exp = 0 present ...
    add(b'{"iat":%d}' % T0)                                        # ... against exp absent
    add(b'{"exp":0,"nbf":0,"iat":0}')
    for claims in (b'{"exp":999999999999999}', b'{"exp":-999999999999999,"nbf":-1,"iat":-5}',
                   b'{"nbf":100000000000000,"exp":1}', b'{"iat":-999999999999999}', b'{"exp":-1}'):
        add(claims)
    for keys in (("ISS", "SUB", "JTI", "AUD", "EXP", "NBF", "IAT"), ("Iss", "sUb", "jtI", "AuD", "eXP", "NbF", "IaT")):
        add(CC.js({k: CC.STD[k.lower()] for k in keys}), CC.FULL)
        add(CC.js({k: CC.STD[k.lower()] for k in keys}), dict(CC.FULL, Subject="other"))
    return out


def write_cases(path, cases):
    """cases [(segment, expected, now_ns)] -> a CASES file of the host programs"""
    sets, index, lines = [], {}, []
    for seg, ex, now_ns in cases:
        key = (repr(sorted(ex.items())), now_ns)
        if key not in index:
            index[key] = len(sets)
            sets.append(CC.resolve(ex, now_ns))
        lines.append("C %d %s\n" % (index[key], CC._hex(seg)))
    with open(path, "w") as f:
        for r in sets:
            f.write("E %s %s %s %d %s%d %d %d %d %d\n" % (
                CC._hex(r["issuer"]), CC._hex(r["subject"]), CC._hex(r["id"]), len(r["audiences"]),
                "".join(CC._hex(a) + " " for a in r["audiences"]), r["now_sec"], r["now_nsec"], r["skew_ns"],
                r["exp_leeway_s"], r["nbf_leeway_s"]))
        f.writelines(lines)


def corpus_cases():
    """the corpus in all_cases() order, as (segment, expected, now_ns)"""
    C = CC.corpus()
    return [(seg,) + tuple(C.sets[si]) for seg, si in C.all_cases()]


def build_host(exe, sanitize=False):
    """Compile tests/host_unit/claims_extract_test.cpp (claims_extract for the CPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the scan's host model"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host_unit", "claims_extract_test.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def run_host(exe, cases_path, env=None):
    """-> (codes [int], records [64 bytes])"""
    r = subprocess.run([exe, cases_path], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    codes, recs = [], []
    for line in r.stdout.splitlines():
        c, h = line.split()
        codes.append(int(c))
        recs.append(bytes.fromhex(h))
    return codes, recs


def unpack(rec: bytes) -> dict:
    return dict(zip(FIELDS, RECORD.unpack(rec)))


def payload_of(seg: bytes) -> bytes:
    return base64.urlsafe_b64decode(seg + b"=" * (-len(seg) % 4))


def claims_of_record(seg: bytes, rec: bytes) -> dict:
    """The jwt.Claims a record stands for, in oracle.jws._claims_struct's form:
    the strings cut from the decoded payload, the dates through `present`."""
    v = unpack(rec)
    payload = payload_of(seg)

    def cut(off, ln):
        assert off + ln <= len(payload), (v, payload)
        return payload[off:off + ln].decode("ascii")
    out = {k: cut(v[k + "_off"], v[k + "_len"]) for k in ("iss", "sub", "jti")}
    text = cut(v["aud_off"], v["aud_len"])
    parts = text.split('"')                        # no escapes: the elements are the quoted runs
    out["aud"] = parts[1::2]
    assert len(out["aud"]) == v["aud_n"], (v, text)
    for bit, k in ((_lib.F_EXP, "exp"), (_lib.F_NBF, "nbf"), (_lib.F_IAT, "iat")):
        if (v["present"] >> bit) & 1:
            out[k] = v[k]
        else:
            assert v[k] == 0, (k, v)
            out[k] = None
    for bit, k in ((_lib.F_ISS, "iss"), (_lib.F_SUB, "sub"), (_lib.F_JTI, "jti"), (_lib.F_AUD, "aud")):
        if not (v["present"] >> bit) & 1:          # absent or null: off / len 0
            assert v[k + "_off"] == 0 and v[k + "_len"] == 0, (k, v)
    if not (v["present"] >> _lib.F_AUD) & 1:
        assert v["aud_n"] == 0, v
    assert v["present"] & ~0xfe == 0, v
    return out


def oracle_struct(seg: bytes) -> dict:
    f, err = jws._claims_struct(jws._claims_map(payload_of(seg)))
    assert err is None, (seg, err)
    return f


def check_records(cases, codes, recs, no_host=False):
    """Every non-HOST record gives the oracle's jwt.Claims; every HOST record is
    64 zero bytes.  Returns the number of decided cases."""
    assert len(cases) == len(codes) == len(recs)
    decided = 0
    for k, ((seg, ex, now_ns), code, rec) in enumerate(zip(cases, codes, recs)):
        assert len(rec) == 64
        if code == _lib.CL_HOST:
            assert not no_host, ("left to the host", k, seg)
            assert rec == bytes(64), ("a HOST record is not zero", k, seg, rec.hex())
            continue
        decided += 1
        got, want = claims_of_record(seg, rec), oracle_struct(seg)
        assert got == want, ("record differs from the oracle's jwt.Claims", k, payload_of(seg), got, want)
    return decided
