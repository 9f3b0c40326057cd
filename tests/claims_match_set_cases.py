"""Shared by the tests of the claims scan with set predicates (claims_match_set /
k_claims_match_set / jg_claims_match_set): the two predicate forms, the sets the
tests ask, the directed list, the sets derived from the corpus, the host build
of tests/host_unit/claims_match_set_test.cpp, and the plain-Python evaluation on
the oracle's claims map.

A predicate is (path, op, value) as in tests/claims_match_hash_cases.py; for
IN_SET and ELEMENT_IN_SET the value is the index of a set of the call (an int).
A call's sets are a list of (members, seed).  Operands are HC's triple (strs,
nums, hashes).

A directed case is D(member, s0, host): the payload {member,"exp":..} with its
operand for one string column; `host` marks the cases the scan leaves to the
host, named one by one.  claims_extract alone decides every other one.
"""
import collections
import functools
import os
import shutil
import subprocess

from cap_amd import _lib
from oracle import jws
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_match_args_cases as AC
from tests import claims_match_cases as MC
from tests import claims_match_hash_cases as HC
from tests import claims_paths_cases as PC
from tests import set_model as SM

ROOT = CC.ROOT
T0 = CC.T0
P = PC.P
IN_SET, ELEMENT_IN_SET = 12, 13                                          # jg_pred_op (include/jg.h)

InSet = lambda path, idx: (path, IN_SET, idx)
ElemIn = lambda path, idx: (path, ELEMENT_IN_SET, idx)
Eq, Has, Elem, EqA, Ge, IsStr = MC.Eq, MC.Has, MC.Elem, AC.EqA, AC.Ge, HC.IsStr

LONG = bytes(0x30 + (7 * j) % 0x4b for j in range(255)).replace(b"\\", b"/")          # a 255-byte member
LONG_OUT = LONG[:254] + b"!"                                                           # ... and a 255-byte non-member


@functools.lru_cache(maxsize=1)
def sets():
    """The four sets of the directed list, each (members, seed): 0 holds revoked ids -- "", a member and its prefix,
    one of a pair of equal hash under its seed, a 255-byte member --, 1 group names, 2 and 3 a few ids of their own"""
    pairs = SM.colliding_pairs()
    return [([b"jti-1", b"", b"abc", b"abcd", pairs[0][0], LONG, b"jti-22", b"s-3", pairs[1][1]] +
             [b"revoked-%d" % k for k in range(40)], SM.SEED),
            ([b"admin", b"ops", b"dev", b" "], 7),
            ([b"jti-2", b"jti-1", b"x"], 0),
            ([b"s3m", b"jti-22"], 0xffffffff)]


def collider():
    """A string that is no member of set 0 and has the 32-bit hash of one"""
    return SM.colliding_pairs()[0][1]


# 0 sid in set 0, 1 groups has an element in set 1, 2 groups in set 1, 3 sid has an element in set 0, 4 sid in set 2 (one
# path, two sets), 5 nonce = s0, 6 n >= 5, 7 sid is a string, 8.. the depths, 11 a.r has an element in set 3 (eight paths)
MAIN = (InSet(P("sid"), 0), ElemIn(P("groups"), 1), InSet(P("groups"), 1), ElemIn(P("sid"), 0), InSet(P("sid"), 2),
        EqA(P("nonce"), 0), Ge(P("n"), 5), IsStr(P("sid")), InSet(P("a", "b", "c", "d"), 0), InSet(P("a", "b"), 0),
        InSet(P("a", "b", "c"), 3), ElemIn(P("a", "r"), 3))
# four sets on one path, by both ops
FOUR = tuple(InSet(P("sid"), x) for x in range(4)) + tuple(ElemIn(P("groups"), x) for x in range(4)) + \
    tuple(ElemIn(P("sid"), x) for x in (0, 3)) + tuple(InSet(P("groups"), x) for x in (1, 2))
# the set ops alone
ONLY = (InSet(P("sid"), 0), ElemIn(P("groups"), 1))
PRED_SETS = collections.OrderedDict([("MAIN", MAIN), ("FOUR", FOUR), ("ONLY", ONLY)])

D = collections.namedtuple("D", "member s0 host", defaults=(b"", False))


@functools.lru_cache(maxsize=1)
def directed_list():
    sid = lambda v: b'"sid":"' + v + b'"'
    grp = lambda v: b'"groups":' + v
    out = []
    # a string in and not in the set; "" in the set; one byte longer and shorter than a member; a member's prefix
    # (itself a member, and not); only the last byte differs; the hash of a member and other bytes
    for v in (b"jti-1", b"jti-2", b"", b"jti-1x", b"jti-", b"abc", b"ab", b"abcd", b"abcde", b"jti-0", b"jti-22", b"jti-23",
              collider(), SM.colliding_pairs()[0][0], SM.colliding_pairs()[1][0], SM.colliding_pairs()[1][1],
              LONG, LONG + b"x", LONG_OUT, LONG[:254], b"x", b"s-3", b"s3m", b"revoked-39", b"revoked-40", b" "):
        out.append(D(sid(v)))
    # a byte >= 0x80: compared raw, never a member
    out += [D(sid(b"jti-\xc3\xa9")), D(sid(b"\xc3\xa9")), D(sid(b"abc\xc2\x80"))]
    # not a string under IN_SET; a string under ELEMENT_IN_SET
    for v in (b"7", b"-0.5", b"null", b"true", b'["jti-1"]', b'{"sid":"jti-1"}', b"[]", b"{}", b'[""]'):
        out.append(D(b'"sid":' + v))
    out += [D(grp(b'"admin"')), D(grp(b'"none"')), D(grp(b'""'))]
    # arrays: no element, one, the first only, the last only, nested containers and other values between
    out += [D(grp(b"[]")), D(grp(b'["admin"]')), D(grp(b'["nobody"]')), D(grp(b'["admin","x","y"]')), D(grp(b'["x","y","admin"]')),
            D(grp(b'["x",["admin"],{"k":"admin"},7,null,true,"y"]')), D(grp(b'["x",["zz"],{"k":"v"},7,null,false,"ops"]')),
            D(grp(b'[["admin"]]')), D(grp(b'[{"admin":"admin"}]')), D(grp(b'[7,"dev",8]')), D(grp(b'[" "]')), D(grp(b'[""]')),
            D(grp(b'[ "x" , "admin" ]')), D(grp(b'["admi","admin ","dmin"]')), D(grp(b'["jti-1","jti-2","s3m"]')),
            D(grp(b'["' + b'","'.join(b"g%d" % k for k in range(40)) + b'","dev"]'))]
    # a key named twice, in both orders; with another type in the place of either
    out += [D(sid(b"jti-1") + b"," + sid(b"nope")), D(sid(b"nope") + b"," + sid(b"jti-1")),
            D(sid(b"jti-1") + b',"sid":7'), D(b'"sid":7,' + sid(b"jti-1")), D(sid(b"jti-1") + b',"sid":null'),
            D(grp(b'["admin"]') + b"," + grp(b'["x"]')), D(grp(b'["x"]') + b"," + grp(b'["admin"]')),
            D(grp(b'["admin"]') + b"," + grp(b'"admin"')), D(grp(b'"admin"') + b"," + grp(b'["x","ops"]'))]
    # depths 1..4, a repeated parent, an array under a path
    d4 = lambda leaf: b'"a":{"b":{"c":{"d":' + leaf + b"}}}"
    out += [D(b'"a":"jti-1"'), D(b'"a":{"b":"jti-1"}'), D(b'"a":{"b":{"c":"s3m"}}'), D(d4(b'"jti-1"')), D(d4(b'"jti-9"')),
            D(d4(b"5")), D(d4(b'"jti-1"') + b',"a":{}'), D(b'"a":{},' + d4(b'"jti-1"')), D(d4(b'"jti-1"') + b',"a":"abc"'),
            D(b'"a":{"b":"jti-1"},"a":{"b":"nope"}'), D(b'"a":{"b":"nope"},"a":{"b":"jti-1"}'),
            D(b'"a":{"b":{"c":"s3m","c":{"d":"abcd"}}}'), D(b'"a":{"r":["q","s3m"]}'), D(b'"a":{"r":"s3m"}'),
            D(b'"a":{"r":["jti-22"],"b":"jti-22"}'), D(b'"a":{"b":[{"c":"s3m"}]}')]
    # beside the older ops in one list: an operand of the token's own, a number, IS_STRING
    out += [D(sid(b"jti-1") + b',"nonce":"n-1","n":5', b"n-1"), D(sid(b"jti-2") + b',"nonce":"n-1","n":4', b"n-2"),
            D(sid(b"jti-1") + b',"nonce":"n-1","n":6,' + grp(b'["ops"]'), b"n-1")]
    # the scan leaves these to the host: an escape in the string
    out += [D(b'"sid":"jti\\u002d1"', host=True), D(grp(b'["ad\\u006din"]'), host=True)]
    return out


@functools.lru_cache(maxsize=1)
def payloads():
    exp = b',"exp":%d}' % (T0 + 5)
    return [b"{" + d.member + exp for d in directed_list()]


@functools.lru_cache(maxsize=1)
def directed():
    """[(segment, expected dict, now_ns)] of payloads()"""
    now = T0 * CC.SECOND
    return [(CC.b64(p), {}, now) for p in payloads()]


def directed_operands():
    """The directed list's own operands: one string column, no number, no hash column"""
    return ([[d.s0 for d in directed_list()]], [], [])


def directed_hosts():
    return {k for k, d in enumerate(directed_list()) if d.host}


# on keys and values the corpus payloads use, older ops among them
CORPUS = (InSet(P("sub"), 0), ElemIn(P("aud"), 1), InSet(P("aud"), 1), InSet(P("iss"), 0), InSet(P("x"), 2),
          InSet(P("deep", "iss"), 0), EqA(P("sub"), 0), Ge(P("exp"), T0), IsStr(P("sub")), InSet(P("jti"), 0),
          ElemIn(P("x"), 2), InSet(P("sub"), 3))
CORPUS_SETS = [CORPUS]


@functools.lru_cache(maxsize=1)
def corpus_sets():
    """Sets from what the corpus payloads hold at the paths CORPUS asks: every other such string (in sorted order) is a
    member, so each predicate holds on some payloads and fails on others"""
    vals = {("sub",): set(), ("iss",): set(), ("jti",): set(), ("aud",): set(), ("x",): set(), ("deep", "iss"): set()}
    for case in XC.corpus_cases():
        claims = AC.claims_of(case[0])
        for path, acc in vals.items():
            present, v = PC.walk(claims, path)
            for e in (v if present and isinstance(v, list) else [v] if present else []):
                if isinstance(e, str) and SM.member_ok(e.encode("utf-8", "surrogatepass")):
                    acc.add(e.encode())
    half = lambda s: sorted(s)[::2]
    s0 = half(vals[("sub",)]) + half(vals[("iss",)]) + half(vals[("jti",)]) + half(vals[("deep", "iss")])
    return [(s0, SM.SEED), (half(vals[("aud",)]), 1), (half(vals[("x",)]) + [b""], 2), (sorted(vals[("sub",)])[1::2], 3)]


def value_bytes(op, value):
    if op in (IN_SET, ELEMENT_IN_SET):
        return bytes([value])
    return HC.value_bytes(op, value)


def split(requires):
    """[(path, op, value)] -> (the distinct paths in order of first use, [(path index, op, value bytes)])"""
    paths, preds = [], []
    for path, op, value in requires:
        if path not in paths:
            paths.append(path)
        preds.append((paths.index(path), op, value_bytes(op, value)))
    return tuple(paths), preds


def build_host(exe, sanitize=False):
    """Compile tests/host_unit/claims_match_set_test.cpp (the scan and set_build for the CPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the scan's host model"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "host_kernels")]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    src = os.path.join(ROOT, "tests", "host_unit", "claims_match_set_test.cpp")
    r = subprocess.run([cxx] + flags + ["-o", exe, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


def write_sets(path, call_sets):
    """[(members, seed)] -> the SETS file of the host program"""
    with open(path, "w") as f:
        for members, seed in call_sets:
            f.write(" ".join(["S", "%d" % seed] + [CC._hex(bytes(m)) if m else "-" for m in members]) + "\n")


def _run(exe, cases_path, args_path, sets_path, paths, preds, env=None):
    return subprocess.run([exe, cases_path, args_path or "-", sets_path or "-"] + MC.raw_args(paths, preds),
                          capture_output=True, text=True, timeout=300, env=env)


def run_host(exe, cases_path, args_path, sets_path, requires, env=None):
    """-> (codes [int], masks [int])"""
    paths, preds = split(requires)
    r = _run(exe, cases_path, args_path, sets_path, paths, preds, env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    codes, masks = [], []
    for line in r.stdout.splitlines():
        c, m = line.split()
        codes.append(int(c))
        masks.append(int(m, 16))
    return codes, masks


def rejected(exe, cases_path, args_path, sets_path, paths, preds):
    """"paths" / "preds" / "sets" / "args <job>" / "hsrc <job>" when the resolve step refuses, else None"""
    r = _run(exe, cases_path, args_path, sets_path, paths, preds)
    assert r.returncode in (0, 3), (r.returncode, r.stderr[-2000:])
    words = r.stdout.split()
    assert (r.returncode == 3) == (words[:1] == ["rejected"])
    return " ".join(words[1:]) if r.returncode == 3 else None


def holds(claims, path, op, value, strs, nums, hs, members):
    """One predicate on a claims map, as Go code on the map decides it; members: one Python set per set of the call"""
    if op < IN_SET:
        return HC.holds(claims, path, op, value, strs, nums, hs)
    present, v = PC.walk(claims, path)
    if not present:
        return False
    raw = lambda s: s.encode("utf-8", "surrogatepass")
    if op == IN_SET:
        return isinstance(v, str) and raw(v) in members[value]
    return isinstance(v, list) and any(isinstance(e, str) and raw(e) in members[value] for e in v)


def evaluate(claims, requires, strs, nums, hs, members):
    return sum(1 << k for k, (path, op, value) in enumerate(requires) if holds(claims, path, op, value, strs, nums, hs, members))


def check(cases, base_codes, codes, masks, requires, operands, call_sets, hosts=None):
    """Codes: claims_extract's (base_codes), or HOST exactly where AC.rule_sends_to_host() says so: the set ops change
    no code.  Masks: evaluate() on the oracle's map for every non-HOST case, 0 for HOST.  With `hosts`: the HOST cases
    are exactly those indices.  Returns (decided, extra HOST)."""
    strs, nums, hashes = operands
    members = [set(bytes(m) for m in ms) for ms, _ in call_sets]
    assert len(cases) == len(base_codes) == len(codes) == len(masks)
    decided = extra = 0
    host = set()
    for k, (case, base, code, mask) in enumerate(zip(cases, base_codes, codes, masks)):
        seg = case[0]
        if base == _lib.CL_HOST:
            assert code == _lib.CL_HOST and mask == 0, (k, seg, code, hex(mask))
            host.add(k)
            continue
        payload = XC.payload_of(seg)
        if AC.rule_sends_to_host(payload, requires):
            assert code == _lib.CL_HOST and mask == 0, ("the rule sends it to the host", k, payload, code, hex(mask))
            extra += 1
            host.add(k)
            continue
        assert code == base, ("the code is not claims_extract's", k, payload, code, base)
        decided += 1
        s, n, h = [col[k] for col in strs], [col[k] for col in nums], [col[k] for col in hashes]
        want = evaluate(jws._claims_map(payload), requires, s, n, h, members)
        assert mask == want, ("mask differs from the evaluation on the oracle's map", k, payload, hex(mask), hex(want))
    if hosts is not None:
        assert host == set(hosts), (sorted(host), sorted(hosts))
    return decided, extra


# ---- what the device tests share ----
OTHER = {"Issuer": "https://other.example/", "Audiences": ["www.example.com"]}
POISON = 0xeeeeeeee


def enc(paths):
    return [[c.encode() if isinstance(c, str) else bytes(c) for c in p] for p in paths]


def assert_same(got, want, what=""):
    n = len(want[0])
    assert len(got[0]) == n and len(got[1]) == n, what
    diff = [k for k in range(n) if got[0][k] != want[0][k] or got[1][k] != want[1][k]]
    assert not diff, (what, [(k, got[0][k], want[0][k], hex(got[1][k]), hex(want[1][k])) for k in diff[:3]])


def assert_host_masks_zero(got, nreq):
    assert all(m == 0 for c, m in zip(*got) if c == _lib.CL_HOST)
    assert all(c <= _lib.CL_HOST for c in got[0])                        # no poison survives
    assert POISON not in got[1] and all(m >> nreq == 0 for m in got[1])


def pool_segments(n):
    """n payload segments drawn from the corpus and from the directed lists of the operand and the select tests"""
    from tests import claims_select_cases as SC
    C = CC.corpus()
    pool = C.plain + C.hard[:200] + [(c[0], 0) for c in AC.directed()] + [(c[0], 0) for c in SC.directed()]
    return [pool[(7 * k) % len(pool)][0] for k in range(n)]


# sixteen predicates of the nine older ops on the keys the pooled payloads use, over eight paths
BATCH = AC.CORPUS_NUM + (AC.EqA(P("sub"), 1), AC.EqA(P("nonce"), 2), AC.Eq(P("nonce"), "abc"), AC.LeA(P("exp"), 3),
                         AC.Elem(P("x"), "y"), AC.Word(P("sub"), "alice@example.com"), AC.Has(P("nonce")))
assert len(BATCH) == 16 and len(AC.split(BATCH)[0]) == 8
