"""Shared by the tests of the path-selecting claims scan (claims_paths_each /
k_claims_paths_each / jg_claims_paths): the directed payload list, the path
sets, the host build of tests/host_unit/claims_paths_test.cpp, and the check of
a jg_selected record against the walk of the oracle's claims map
(oracle.jws._claims_map) along each path.

The corpus itself is tests/claims_corpus.py's.  The directed payloads hold no
escapes and integer dates, so the scan decides every one of them (HOST == 0);
they are crossed with every path set of PATH_SETS.
"""
import functools
import os
import shutil
import subprocess

from cap_amd import _lib
from oracle import jws
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_select_cases as SC

ROOT = CC.ROOT
T0 = CC.T0
LONG = SC.LONG                               # a component of JG_SELECT_NAME_MAX bytes

P = lambda *c: tuple(c)
# eight paths: depths 1..4, shared prefixes, a path that is a prefix of another
EIGHT = (P("realm_access", "roles"), P("realm_access", "groups"), P("realm_access"), P("cnf", "jkt"),
         P("resource_access", "app", "roles"), P("act", "sub"), P("a", "b", "c", "d"), P("scope"))
AB = (P("a", "b"),)
PREFIXES = (P("a"), P("a", "b"), P("a", "b", "c"), P("a", "b", "c", "d"))
ROLE = (P("a", "role"), P("a", "roles"), P("a", "r"), P("role", "a"), P("roles", "a"))
TYPES = tuple(P("t", n) for n in ("str", "raw", "num", "yes", "no", "nil", "arr", "obj"))
LONGS = (P(LONG, LONG), P("k", LONG, "k"))
PATH_SETS = [(), (P("scope"),), AB, EIGHT, PREFIXES, ROLE, TYPES, LONGS, (P("a", "b"), P("a", "c"), P("b", "a"))]
# a one-component path set is the name set, slot for slot
ONE_COMPONENT = [tuple(P(n) for n in names) for names in SC.NAME_SETS]

# keys the corpus payloads (tests/claims_corpus.py) use, at depth 1 and deeper
CORPUS_SETS = [(), (P("x"),), tuple(P(n) for n in SC.CORPUS_NAMES),
               (P("deep", "a"), P("a", "b"), P("x", "a"), P("b", "a", "x"), P("deep"), P("a"), P("name", "x"), P("aud", "a"))]


@functools.lru_cache(maxsize=1)
def payloads():
    """The directed payloads: every one is decided by the scan."""
    out = []
    exp = b'"exp":%d' % (T0 + 5)
    # the contract's cases, for a/b
    out += [b'{"a":{"b":1},"a":{},' + exp + b"}",                      # the later parent replaces the earlier one
            b'{"a":{"b":1},"a":5,' + exp + b"}",
            b'{"a":{"b":1},"a":null,' + exp + b"}",
            b'{"a":{"b":1},"a":[{"b":2}],' + exp + b"}",
            b'{"a":{"b":1},"a":"b",' + exp + b"}",
            b'{"a":{},"a":{"b":1},' + exp + b"}",
            b'{"a":5,"a":{"b":"second"},' + exp + b"}",
            b'{"a":{"b":1,"b":[2]},' + exp + b"}",                      # the last member
            b'{"a":{"b":[2],"x":0,"b":"s"},' + exp + b"}",
            b'{"a":null,' + exp + b"}",
            b'{"a":[{"b":1}],' + exp + b"}",                            # arrays are never descended
            b'{"a":[[{"b":1}]],' + exp + b"}",
            b'{"x":{"a":{"b":1}},' + exp + b"}",                        # component j sits at depth j
            b'{"b":1,"a":{"x":{"b":2}},' + exp + b"}",
            b'{"a":{"x":{"b":2},"b":3},' + exp + b"}",                  # back from a deeper object
            b'{"a":{"x":[{"b":2}],"b":{"b":4}},' + exp + b"}",
            b'{"a":{"a":{"b":1}},' + exp + b"}",
            b'{"a":{"b":{"a":{"b":7}}},"b":{"a":1},' + exp + b"}",
            b'{"a":{"c":1},"b":{"a":2,"b":3},' + exp + b"}",
            b'{"a" : { "b" :\t[ 1 , 2 ] } , ' + exp + b" }",
            b"{" + exp + b',"a":{"b":-0.5}}',                            # a number ended by the parent's }, then the root's
            b"{" + exp + b',"a":{"b":7} }',
            b"{" + exp + b',"a":{"b":{}}}']
    # shared prefixes, a prefix of another, all eight slots, each at depth 1..4
    out += [b'{"realm_access":{"roles":["admin","dev"],"groups":["/g"]},"cnf":{"jkt":"0ZcOCORZNYy"},'
            b'"resource_access":{"app":{"roles":["r1"]},"other":{"roles":["no"]}},"act":{"sub":"svc"},'
            b'"a":{"b":{"c":{"d":[4]}}},"scope":"a b","sub":"alice@example.com","iat":%d}' % T0,
            b'{"realm_access":{"groups":[]},"resource_access":{"app":{}},"act":{"sub":null,"act":{"sub":"inner"}},'
            + exp + b"}",
            b'{"realm_access":{"roles":"r"},"realm_access":{"groups":"g"},' + exp + b"}",
            b'{"cnf":{"x5t#S256":"t","jkt":"j"},"cnf":{"jkt":"k","jkt":"l"},' + exp + b"}"]
    # depth 4, and a four-component path inside a depth-5 object
    out += [b'{"a":{"b":{"c":{"d":1}}},' + exp + b"}",
            b'{"a":{"b":{"c":{"d":{"e":{"f":[]}}}}},' + exp + b"}",
            b'{"a":{"b":{"c":{"d":{"d":5}},"c":{"x":1}}},' + exp + b"}",      # a/b/c replaced: a/b/c/d absent
            b'{"a":{"b":{"c":{"d":"deep"},"x":{"c":{"d":0}}}},' + exp + b"}",
            b'{"a":{"b":{"c":[{"d":1}]}},' + exp + b"}",
            b'{"z":{"a":{"b":{"c":{"d":1}}}},' + exp + b"}",
            b'{"a":{"b":{"c":{"d":1}},"b":3},' + exp + b"}",
            b'{"a":{"b":{"c":{"d":true,"d":false}}}}']
    # components that are prefixes of each other, near misses, casing
    out += [b'{"a":{"r":1,"roles":[2],"role":"three","ro":4,"rolesx":5},"role":{"a":6},"roles":{"a":null},' + exp + b"}",
            b'{"a":{"roles":"only the longer one"},"roles":{"ab":1},' + exp + b"}",
            b'{"a":{"Role":1,"ROLES":2},"A":{"role":3},' + exp + b"}"]
    # a nested key with a byte >= 0x80 beside a matching one
    out += ['{"a":{"rôle":1,"role":2,"rolesé":3,"é":{"role":4}},'.encode() + exp + b"}",
            b'{"a":{"\xff":1,"b":"after","b\xff":2},' + exp + b"}",
            '{"a":{"b":"Jürgen"},'.encode() + exp + b"}"]
    # 64-byte components, with neighbours of 63 and 65 bytes
    L = LONG.encode()
    out += [b'{"' + L + b'":{"' + L[:63] + b'":63,"' + L + b'":"long","' + L + b'L":65},"k":{"' + L + b'":{"k":[1]}},'
            + exp + b"}"]
    # every jg_sel_type at depth 2, the value at every decoded position mod 3
    for shift in range(3):
        pad = b"x" * shift
        out.append(b'{"p":"' + pad + b'","t":{"str":"s","raw":"\xc3\xa9","num":-12.25,"yes":true,"no":false,"nil":null,'
                   b'"arr":[1,{"str":2}],"obj":{"str":{}}},' + exp + b"}")
        out.append(b'{"p":"' + pad + b'","a":{"b":"v"},' + exp + b"}")
        out.append(b'{"p":"' + pad + b'","a":{"b":{"c":{"d":12345678901234567}}},' + exp + b"}")
    # a top-level name list's payloads: one-component paths are jg_claims_select's slots
    out += [b'{"scope":"first","scope":[1,2],' + exp + b"}", b'{"scope":{"scope":"inner"},' + exp + b"}",
            b"{" + exp + b"}", b"{}"]
    return out


@functools.lru_cache(maxsize=1)
def directed():
    """[(segment, expected dict, now_ns)] of payloads()"""
    now = T0 * CC.SECOND
    return [(CC.b64(p), CC.FULL if b"alice" in p else {}, now) for p in payloads()]


def build_host(exe, sanitize=False):
    """Compile tests/host_unit/claims_paths_test.cpp (claims_paths_each for the CPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the scan's host model"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host_unit", "claims_paths_test.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


def _b(c):
    return c.encode() if isinstance(c, str) else bytes(c)


def path_args(paths):
    return ["/".join(CC._hex(_b(c)) for c in p) if len(p) else "@" for p in paths]


def run_host(exe, cases_path, paths, env=None):
    """-> (codes [int], jg_claims records [64 bytes], jg_selected records [80 bytes])"""
    r = subprocess.run([exe, cases_path] + path_args(paths), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    codes, recs, sels = [], [], []
    for line in r.stdout.splitlines():
        c, h, q = line.split()
        codes.append(int(c))
        recs.append(bytes.fromhex(h))
        sels.append(bytes.fromhex(q))
    return codes, recs, sels


def rejected(exe, cases_path, paths):
    """True when resolve_paths() refuses the path list"""
    r = subprocess.run([exe, cases_path] + path_args(paths), capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), (r.returncode, r.stderr[-2000:])
    assert (r.returncode == 3) == (r.stdout.strip() == "rejected")
    return r.returncode == 3


def walk(claims, path):
    """(present, value): the claims map walked along the path, as Go code would"""
    cur = claims
    for c in path:
        if not isinstance(cur, dict) or c not in cur:
            return False, None
        cur = cur[c]
    return True, cur


def check_selected(cases, codes, sels, paths, no_host=False):
    """Every non-HOST jg_selected, cut out of the decoded payload, gives the walk
    of oracle.jws._claims_map(payload) along each path; every HOST record is 80
    zero bytes.  Returns the number of decided cases."""
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
        v = SC.unpack(sel)
        assert v["pad"] == bytes(8), (k, sel.hex())
        payload = XC.payload_of(seg)
        claims = jws._claims_map(payload)
        for s in range(8):
            present, got = SC.value_of(payload, v["off"][s], v["len"][s], v["type"][s])
            if s >= len(paths):
                assert not present, ("a slot past the paths is filled", k, s, sel.hex())
                continue
            wp, want = walk(claims, paths[s])
            assert present == wp, ("presence differs", k, paths[s], payload, v)
            if present:
                assert SC.same(got, want), ("value differs from the oracle's walk", k, paths[s], payload, got, want)
    return decided
