"""Shared by the tests of the selecting claims scan (claims_select /
k_claims_select / jg_claims_select): the directed payload list, the name sets,
the host build of tests/host_unit/claims_select_test.cpp, and the check of a
jg_selected record against the oracle's claims map (oracle.jws._claims_map).

The corpus itself is tests/claims_corpus.py's.  The directed payloads hold no
escapes and integer dates, so the scan decides every one of them (HOST == 0);
they are crossed with every name set of NAME_SETS.
"""
import functools
import os
import shutil
import struct
import subprocess

from cap_amd import _lib
from oracle import jws
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC

ROOT = CC.ROOT
T0 = CC.T0
SELECTED = struct.Struct("<8I8I8B8s")        # jg_selected (include/jg.h)
assert SELECTED.size == 80

LONG = "L" * 64                              # a name of JG_SELECT_NAME_MAX bytes
EIGHT = ("scope", "roles", "tenant", "email", "nonce", "azp", "auth_time", "sub")
# sizes 0, 1 and 8; names that are prefixes of each other; 1 and 64 bytes; a
# name that differs from the payloads' key only in case; a registered name
NAME_SETS = [(), ("scope",), EIGHT, ("scope", "scopes", "s"), ("k", LONG), ("Scope",), ("sub", "scope")]

# keys the corpus payloads (tests/claims_corpus.py) use, at depth 1 and deeper: a set of 8
CORPUS_NAMES = ("iss", "aud", "exp", "deep", "name", "x", "a", "b")

LITERAL = {_lib.SEL_TRUE: (b"true", True), _lib.SEL_FALSE: (b"false", False), _lib.SEL_NULL: (b"null", None)}


@functools.lru_cache(maxsize=1)
def payloads():
    """The directed payloads: every one is decided by the scan."""
    out = []
    exp = b'"exp":%d' % (T0 + 5)
    values = [b'"x"', b'""', b"[]", b"{}", b"-0", b"0", b"1.5", b"12345678901234567", b"-12.25", b"true", b"false",
              b"null", b'["a",{"b":[1,2]},[]]', b'{"a":{"b":1},"c":[{}]}', b'"a}b]c,d:e{["', b'"read write"']
    for v in values:
        out.append(b'{"scope":' + v + b"," + exp + b"}")                      # first, followed by ,
        out.append(b"{" + exp + b',"scope":' + v + b',"z":1}')               # in the middle
        out.append(b"{" + exp + b',"scope":' + v + b"}")                      # last, followed by }
        for ws in (b" ", b"\t", b"\n", b"\r"):
            out.append(b'{"scope":' + v + ws + b"," + exp + b"}")
            out.append(b"{" + exp + b',"scope":' + v + ws + b"}")
        out.append(b'{ "scope" \t:\r\n ' + v + b" , " + exp + b" }")
        for shift in range(3):                                               # the value at every decoded position mod 3
            out.append(b'{"p":"' + b"x" * shift + b'","scope":' + v + b"," + exp + b"}")
    # the selected key again at depth 2: no match there, the outer span undisturbed
    out += [b'{"o":{"scope":"inner","x":{"scope":2}},"scope":"outer",' + exp + b"}",
            b'{"scope":"outer","o":{"scope":"inner"},' + exp + b"}",
            b'{"scope":{"scope":"inner"},' + exp + b"}",
            b'{"scope":[{"scope":1},"scope"],' + exp + b"}",
            b'{"o":[{"scope":[1]}],' + exp + b"}"]
    # the name twice at depth 1: the last wins, with different types in the two places
    out += [b'{"scope":"first","scope":[1,2],' + exp + b"}",
            b'{"scope":[1],' + exp + b',"scope":7}',
            b'{"scope":{"a":1},"scope":null,' + exp + b"}",
            b'{"scope":1,"x":0,"scope":"s"}',
            b'{"scope":"a long first value","scope":""}']
    # STRING_RAW: valid UTF-8 and a lone 0xff
    out += ['{"scope":"J\u00fcrgen \u4e2d",'.encode() + exp + b"}", b'{"scope":"a\xffb",' + exp + b"}",
            b"{" + exp + b',"scope":"\xff"}']
    # names that are prefixes of each other, and near misses
    out += [b'{"s":1,"scopes":[2],"scope":"three","sc":4,"scopex":5,' + exp + b"}",
            b'{"scopes":"only the longer one",' + exp + b"}"]
    # casing
    out += [b'{"Scope":"upper","scope":"lower",' + exp + b"}", b'{"SCOPE":1,' + exp + b"}"]
    # a registered name: exact in the slot, any casing for the registered logic
    out += [b'{"SUB":"alice@example.com",' + exp + b"}", b'{"sub":"bob",' + exp + b"}", b'{"sub":null,' + exp + b"}"]
    # 1 byte and 64 bytes, with neighbours of 63 and 65
    out += [b'{"k":1,"' + LONG.encode() + b'":"long","' + LONG[:63].encode() + b'":63,"' + LONG.encode() + b'L":65,'
            + exp + b"}"]
    # all eight present, each type once
    out += [b'{"scope":"a b","roles":["admin","dev"],"tenant":{"id":7},"email":"a@b.c","nonce":"n-1","azp":null,'
            b'"auth_time":1611699000,"sub":"alice@example.com","iat":%d}' % T0]
    # none present
    out += [b"{" + exp + b"}", b"{}", b'{"other":[1,2,3],' + exp + b"}"]
    return out


@functools.lru_cache(maxsize=1)
def directed():
    """[(segment, expected dict, now_ns)] of payloads()"""
    now = T0 * CC.SECOND
    return [(CC.b64(p), CC.FULL if b"alice" in p else {}, now) for p in payloads()]


def host_only():
    """Next to the directed list, but the scan's rules leave it to the host"""
    now = T0 * CC.SECOND
    return [(CC.b64(b'{"scope":123456789012345678,"exp":%d}' % (T0 + 5)), {}, now)]


def build_host(exe, sanitize=False):
    """Compile tests/host_unit/claims_select_test.cpp (claims_select for the CPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the scan's host model"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host_unit", "claims_select_test.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


def name_args(names):
    return [CC._hex(n.encode() if isinstance(n, str) else bytes(n)) for n in names]


def run_host(exe, cases_path, names, env=None):
    """-> (codes [int], jg_claims records [64 bytes], jg_selected records [80 bytes])"""
    r = subprocess.run([exe, cases_path] + name_args(names), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    codes, recs, sels = [], [], []
    for line in r.stdout.splitlines():
        c, h, q = line.split()
        codes.append(int(c))
        recs.append(bytes.fromhex(h))
        sels.append(bytes.fromhex(q))
    return codes, recs, sels


def rejected(exe, cases_path, names):
    """True when resolve_select() refuses the name list"""
    r = subprocess.run([exe, cases_path] + name_args(names), capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), (r.returncode, r.stderr[-2000:])
    assert (r.returncode == 3) == (r.stdout.strip() == "rejected")
    return r.returncode == 3


def unpack(sel: bytes) -> dict:
    v = SELECTED.unpack(sel)
    return {"off": v[0:8], "len": v[8:16], "type": v[16:24], "pad": v[24]}


def value_of(payload: bytes, off: int, ln: int, typ: int):
    """The Go value a slot stands for: (present, value), cut from the decoded payload"""
    if typ == _lib.SEL_ABSENT:
        assert off == 0 and ln == 0
        return False, None
    assert off + ln <= len(payload), (off, ln, payload)
    text = payload[off:off + ln]
    if typ == _lib.SEL_STRING:
        assert payload[off - 1:off] == b'"' and payload[off + ln:off + ln + 1] == b'"', (text, payload)
        assert all(c < 0x80 for c in text)
        return True, text.decode("ascii")
    if typ == _lib.SEL_STRING_RAW:
        assert text[:1] == b'"' and text[-1:] == b'"' and any(c >= 0x80 for c in text), text
        return True, jws.go_json(text)
    if typ == _lib.SEL_NUMBER:
        assert 0 < ln <= 17 and text[:1] in b"-0123456789", text
        return True, float(text)
    if typ in LITERAL:
        assert text == LITERAL[typ][0], text
        return True, LITERAL[typ][1]
    assert typ in (_lib.SEL_ARRAY, _lib.SEL_OBJECT), typ
    assert (text[:1], text[-1:]) == ((b"[", b"]") if typ == _lib.SEL_ARRAY else (b"{", b"}")), text
    return True, jws.go_json(text)


def same(a, b):
    """Equal as Go values: floats by their 8 bytes (-0.0 is not 0.0), bools are not numbers"""
    if type(a) is not type(b):
        return False
    if isinstance(a, float):
        return struct.pack("<d", a) == struct.pack("<d", b)
    if isinstance(a, list):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return a == b


def check_selected(cases, codes, sels, names, no_host=False):
    """Every non-HOST jg_selected, cut out of the decoded payload, gives
    oracle.jws._claims_map(payload).get(name) for each name; every HOST record is
    80 zero bytes.  Returns the number of decided cases."""
    assert len(cases) == len(codes) == len(sels)
    decided = 0
    for k, (case, code, sel) in enumerate(zip(cases, codes, sels)):
        seg = case[0]
        assert len(sel) == 80
        if code == _lib.CL_HOST:
            assert not no_host, ("left to the host", k, seg)
            assert sel == bytes(80), ("a HOST record is not zero", k, seg, sel.hex())
            continue
        decided += 1
        v = unpack(sel)
        assert v["pad"] == bytes(8), (k, sel.hex())
        payload = XC.payload_of(seg)
        want = jws._claims_map(payload)
        for s in range(8):
            present, got = value_of(payload, v["off"][s], v["len"][s], v["type"][s])
            if s >= len(names):
                assert not present, ("a slot past the names is filled", k, s, sel.hex())
                continue
            assert present == (names[s] in want), ("presence differs", k, names[s], payload, v)
            if present:
                assert same(got, want[names[s]]), ("value differs from the oracle's map", k, names[s], payload, got,
                                                   want[names[s]])
    return decided
