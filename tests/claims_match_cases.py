"""Shared by the tests of the predicate-matching claims scan (claims_match_each /
k_claims_match_each / jg_claims_match): the directed payload list, the
predicate sets, the host build of tests/host_unit/claims_match_test.cpp, and the
plain-Python evaluation of a predicate on the oracle's claims map
(oracle.jws._claims_map, walked with claims_paths_cases.walk).

A predicate is written (path, op, value) with the path a tuple of components;
split() turns a list of them into the ABI's form: the distinct paths and, per
predicate, the index of its path.

The corpus itself is tests/claims_corpus.py's.  The directed payloads hold no
escapes and integer dates, so the scan decides every one of them (HOST == 0);
they are crossed with every predicate set of PRED_SETS.
"""
import functools
import os
import shutil
import subprocess

from cap_amd import _lib
from oracle import jws
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_paths_cases as PC

ROOT = CC.ROOT
T0 = CC.T0
P = PC.P
EQUALS, HAS_WORD, HAS_ELEMENT, PRESENT = 1, 2, 3, 4            # jg_pred_op (include/jg.h)
V64 = "v" * 64                                                # a value of JG_PRED_VALUE_MAX bytes

Eq = lambda path, v: (path, EQUALS, v)
Word = lambda path, v: (path, HAS_WORD, v)
Elem = lambda path, v: (path, HAS_ELEMENT, v)
Has = lambda path: (path, PRESENT, "")

ROLES = (Elem(P("roles"), "admin"), Elem(P("roles"), "user"), Has(P("roles")), Eq(P("roles"), "admin"),
         Word(P("roles"), "admin"))
AR = (Elem(P("a", "r"), "x"), Has(P("a", "r")), Has(P("a")), Eq(P("a", "r"), "x"))
SCOPE = (Word(P("scope"), "read"), Word(P("scope"), "read:all"), Eq(P("scope"), "read"), Eq(P("scope"), ""),
         Eq(P("scope"), "read write"), Has(P("scope")), Elem(P("scope"), "read"), Word(P("scope"), "write"),
         Eq(P("scope"), " read"))
LONGV = (Eq(P("k"), V64), Elem(P("k"), V64), Word(P("k"), V64), Eq(P("k"), V64[:63]))
DEEP = (Elem(P("a", "b", "c", "d"), "z"), Has(P("a", "b", "c", "d")), Has(P("a", "b", "c")),
        Eq(P("a", "b", "c", "d"), "z"), Eq(P("a", "b", "c", "d"), "deep"))
REGISTERED = (Elem(P("aud"), "www.example.com"), Eq(P("aud"), "www.example.com"), Eq(P("sub"), "alice@example.com"),
              Word(P("sub"), "alice@example.com"), Has(P("exp")), Elem(P("aud"), "b"))
ENCLOSING = (Has(P("realm_access")), Elem(P("realm_access", "roles"), "admin"), Has(P("realm_access", "roles")),
             Elem(P("realm_access", "roles"), "dev"), Elem(P("realm_access", "groups"), "/g"))
# all sixteen predicates over the eight paths of claims_paths_cases.EIGHT
FULL = (Elem(PC.EIGHT[0], "admin"), Elem(PC.EIGHT[0], "dev"), Elem(PC.EIGHT[1], "/g"), Has(PC.EIGHT[2]),
        Eq(PC.EIGHT[3], "0ZcOCORZNYy"), Has(PC.EIGHT[3]), Elem(PC.EIGHT[4], "r1"), Elem(PC.EIGHT[4], "no"),
        Eq(PC.EIGHT[5], "svc"), Has(PC.EIGHT[5]), Elem(PC.EIGHT[6], "4"), Has(PC.EIGHT[6]),
        Word(PC.EIGHT[7], "a"), Word(PC.EIGHT[7], "b"), Eq(PC.EIGHT[7], "a b"), Word(PC.EIGHT[7], "a_b"))
assert len(FULL) == 16
PRED_SETS = [(), ROLES, AR, SCOPE, LONGV, DEEP, REGISTERED, ENCLOSING, FULL]

# predicates on keys and values the corpus payloads (tests/claims_corpus.py) use
CORPUS_SETS = [(),
               (Has(P("x")), Eq(P("x"), "y"), Has(P("deep")), Has(P("deep", "a")), Elem(P("aud"), "www.example.com"),
                Eq(P("aud"), "www.example.com"), Eq(P("iss"), "https://example.com/"), Has(P("exp"))),
               (Eq(P("name"), ""), Word(P("name"), "a"), Elem(P("a"), "b"), Has(P("a", "b")), Eq(P("sub"), "alice@example.com"),
                Word(P("iss"), "https://example.com/"), Elem(P("b"), "a"), Has(P("b", "a", "x")), Has(P("a")),
                Has(P("b")), Has(P("name")), Elem(P("x"), "y"), Eq(P("x"), "y"), Eq(P("a"), "b"))]


def split(requires):
    """[(path, op, value)] -> (the distinct paths in order of first use, [(path index, op, value bytes)])"""
    paths, preds = [], []
    for path, op, value in requires:
        if path not in paths:
            paths.append(path)
        preds.append((paths.index(path), op, value.encode() if isinstance(value, str) else bytes(value)))
    return tuple(paths), preds


@functools.lru_cache(maxsize=1)
def payloads():
    """The directed payloads: every one is decided by the scan."""
    out = []
    exp = b'"exp":%d' % (T0 + 5)
    wrap = lambda member: b"{" + member + b"," + exp + b"}"
    # the last member wins
    out += [wrap(b'"roles":["admin"],"roles":["user"]'), wrap(b'"roles":["user"],"roles":["admin"]'),
            wrap(b'"roles":["admin"],"roles":"admin"'), wrap(b'"roles":"admin","roles":null'),
            wrap(b'"roles":["admin"],"x":1,"roles":[]')]
    # a replaced parent, a key at the wrong depth
    out += [wrap(b'"a":{"r":["x"]},"a":{}'), wrap(b'"a":{"r":["x"]},"a":5'), wrap(b'"a":{},"a":{"r":["x"]}'),
            wrap(b'"a":{"r":["x"]}'), wrap(b'"a":{"r":["x"]},"a":{"r":"x"}'), wrap(b'"a":{"r":"x","r":["y"]}'),
            wrap(b'"a":{"r":["x"]},"a":[{"r":["x"]}]'), wrap(b'"a":{"r":null},"b":{"r":["x"]}'),
            wrap(b'"x":{"roles":["admin"]}'), wrap(b'"x":[{"roles":["admin"]}],"r":["x"]')]
    # prefix and suffix traps
    out += [wrap(b'"roles":["administrator","adm","xadmin","admiN"]'),
            wrap(b'"roles":["administrator","adm","xadmin","admiN","admin"]'),
            wrap(b'"roles":"administrator"'), wrap(b'"roles":"adm"'), wrap(b'"roles":"xadmin"'), wrap(b'"roles":"admiN"'),
            wrap(b'"scope":"read:all"'), wrap(b'"scope":"thread"'), wrap(b'"scope":"write read"'),
            wrap(b'"scope":"read:all read"'), wrap(b'"scope":"read read:all"'), wrap(b'"scope":"rea"'),
            wrap(b'"scope":"reads"'), wrap(b'"scope":"read:al read:allx"')]
    # HAS_WORD: spaces at either end and doubled, "", one word, bytes >= 0x80 beside a match
    out += [wrap(b'"scope":" read"'), wrap(b'"scope":"read "'), wrap(b'"scope":"a  read"'), wrap(b'"scope":"  "'),
            wrap(b'"scope":" "'), wrap(b'"scope":""'), wrap(b'"scope":"read"'), wrap(b'"scope":"read write"'),
            wrap('"scope":"réad read"'.encode()), wrap('"scope":"réad"'.encode()),
            wrap(b'"scope":"re\xffad write"'), wrap(b'"scope":"read\xc2\xa0write"'), wrap(b'"scope":"\xff read"'),
            wrap(b'"scope":["read"]'), wrap(b'"scope":null'), wrap(b'"scope":17'), wrap(b'"scope":{"read":"read"}')]
    # HAS_ELEMENT
    out += [wrap(b'"roles":[]'), wrap(b'"roles":[1,null,true,false,-2.5]'), wrap(b'"roles":[["admin"]]'),
            wrap(b'"roles":[{"admin":"admin"}]'), wrap(b'"roles":["x",["y"],"admin"]'),
            wrap(b'"roles":["x",{"k":["z"]},"admin"]'), wrap(b'"roles":"admin"'),
            wrap('"roles":["admín","admin"]'.encode()), wrap('"roles":["admín"]'.encode()),
            wrap(b'"roles":[ "user" , "admin" ]'), wrap(b'"roles":[[],{},"user"]'), wrap(b'"roles":["",1,"admin"]'),
            wrap(b'"roles":[{"roles":["admin"]},["admin",["admin"]]]'), wrap(b'"roles":["admin user"]')]
    # EQUALS: "", an array, the longest value against its neighbours
    v = V64.encode()
    out += [wrap(b'"k":"' + v + b'"'), wrap(b'"k":"' + v + b'v"'), wrap(b'"k":"' + v[:63] + b'"'),
            wrap(b'"k":["' + v + b'v","' + v + b'"]'), wrap(b'"k":"x ' + v + b'"'), wrap(b'"k":"' + v + b' ' + v[:63] + b'"'),
            wrap(b'"k":""'), wrap(b'"k":[""]')]
    # PRESENT: null, absent; depth 4
    out += [wrap(b'"a":null'), wrap(b'"a":{"r":null}'), wrap(b'"b":1'),
            wrap(b'"a":{"b":{"c":{"d":["y","z"]}}}'), wrap(b'"a":{"b":{"c":{"d":"z"}}}'),
            wrap(b'"a":{"b":{"c":{"d":[{"d":["z"]}]}}}'), wrap(b'"a":{"b":{"c":{"d":["z"]},"c":{}}}'),
            wrap(b'"a":{"b":{"c":{"d":["y",["z"],{"d":"z"},"z"]}}}')]
    # registered names as paths
    out += [b'{"aud":"www.example.com","sub":"alice@example.com",' + exp + b"}",
            b'{"aud":["b","www.example.com"],"sub":"alice@example.com",' + exp + b"}",
            b'{"aud":[],"sub":"bob",' + exp + b"}",
            CC.js(CC.STD)]
    # a failure code with a filled mask
    out += [b'{"roles":["admin"],"scope":"read","exp":%d}' % (T0 - 86400),
            b'{"realm_access":{"roles":["admin"]},"iat":%d}' % (T0 + 86400)]
    return out + PC.payloads()


@functools.lru_cache(maxsize=1)
def directed():
    """[(segment, expected dict, now_ns)] of payloads()"""
    now = T0 * CC.SECOND
    return [(CC.b64(p), CC.FULL if b"alice" in p else {}, now) for p in payloads()]


def build_host(exe, sanitize=False):
    """Compile tests/host_unit/claims_match_test.cpp (claims_match_each for the CPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the scan's host model"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host_unit", "claims_match_test.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


def pred_args(preds):
    return ["%d:%d:%s" % (path, op, CC._hex(value)) for path, op, value in preds]


def raw_args(paths, preds):
    """the program's arguments for paths and predicates already in the ABI's form"""
    return PC.path_args(paths) + ["--"] + pred_args(preds)


def run_host(exe, cases_path, requires, env=None):
    """-> (codes [int], masks [int])"""
    paths, preds = split(requires)
    r = subprocess.run([exe, cases_path] + raw_args(paths, preds), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    codes, masks = [], []
    for line in r.stdout.splitlines():
        c, m = line.split()
        codes.append(int(c))
        masks.append(int(m, 16))
    return codes, masks


def rejected(exe, cases_path, paths, preds):
    """"paths" / "preds" when resolve_paths() / resolve_preds() refuses the list, else None"""
    r = subprocess.run([exe, cases_path] + raw_args(paths, preds), capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), (r.returncode, r.stderr[-2000:])
    words = r.stdout.split()
    assert (r.returncode == 3) == (words[:1] == ["rejected"])
    return words[1] if r.returncode == 3 else None


def holds(claims, path, op, value):
    """One predicate on a claims map, as Go code on the map ValidateBatch builds would decide it"""
    present, v = PC.walk(claims, path)
    if not present:
        return False
    if op == PRESENT:
        return True
    if op == EQUALS:
        return isinstance(v, str) and v == value
    if op == HAS_WORD:
        return isinstance(v, str) and value in v.split(" ")
    if op == HAS_ELEMENT:
        return isinstance(v, list) and any(isinstance(e, str) and e == value for e in v)
    raise ValueError(op)


def evaluate(claims, requires):
    """The mask jg_claims_match owes for the claims map"""
    return sum(1 << k for k, (path, op, value) in enumerate(requires) if holds(claims, path, op, value))


def check_masks(cases, codes, masks, requires, no_host=False):
    """Every non-HOST mask is evaluate() on oracle.jws._claims_map(payload); every
    HOST mask is 0.  Returns the number of decided cases."""
    assert len(cases) == len(codes) == len(masks)
    decided = 0
    for k, (case, code, mask) in enumerate(zip(cases, codes, masks)):
        seg = case[0]
        if code == _lib.CL_HOST:
            assert not no_host, ("left to the host", k, seg)
            assert mask == 0, ("a HOST mask is not zero", k, seg, hex(mask))
            continue
        decided += 1
        payload = XC.payload_of(seg)
        want = evaluate(jws._claims_map(payload), requires)
        assert mask == want, ("mask differs from the evaluation on the oracle's map", k, payload, hex(mask), hex(want), requires)
    return decided
