"""Shared by the tests of the claims scan with per-token operands and numeric
tests (claims_match_args / k_claims_match_args / jg_claims_match_args): the
predicate forms, the directed list with its operands, the derivation of operands
for the corpus, the host build of tests/host_unit/claims_match_args_test.cpp, and
the plain-Python evaluation on the oracle's claims map.

A predicate is (path, op, value) as in tests/claims_match_cases.py; for the new
ops the value is the column (an int) or the bound (an int).  Operands are a pair
(strs, nums): lists of columns, each with one entry per case.

A directed case is D(member, s0, s1, n0, n1, host): the payload {member,"exp":..}
with its own operands for two string and two number columns, and the names of
the predicate sets under which the rule of include/jg.h sends it to the host (a
number of another form than -?(0|[1-9][0-9]{0,14}) on the full path of a numeric
predicate).  claims_extract alone decides every directed payload.
"""
import collections
import functools
import json
import os
import re
import shutil
import struct
import subprocess

from cap_amd import _lib
from oracle import jws
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_match_cases as MC
from tests import claims_paths_cases as PC

ROOT = CC.ROOT
T0 = CC.T0
P = PC.P
EQUALS, HAS_WORD, HAS_ELEMENT, PRESENT = MC.EQUALS, MC.HAS_WORD, MC.HAS_ELEMENT, MC.PRESENT
EQUALS_ARG, NUM_GE, NUM_LE, NUM_GE_ARG, NUM_LE_ARG = 5, 6, 7, 8, 9          # jg_pred_op (include/jg.h)
NUMERIC = (NUM_GE, NUM_LE, NUM_GE_ARG, NUM_LE_ARG)
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
DATE_FORM = re.compile(rb"-?(0|[1-9][0-9]{0,14})")

Eq, Word, Elem, Has = MC.Eq, MC.Word, MC.Elem, MC.Has
EqA = lambda path, col: (path, EQUALS_ARG, col)
Ge = lambda path, n: (path, NUM_GE, n)
Le = lambda path, n: (path, NUM_LE, n)
GeA = lambda path, col: (path, NUM_GE_ARG, col)
LeA = lambda path, col: (path, NUM_LE_ARG, col)

# 0 nonce = s0, 1 nonce = "abc", 2 nonce = s1, 3 present: ARG and constant EQUALS and two columns on one path
NONCE = (EqA(P("nonce"), 0), Eq(P("nonce"), "abc"), EqA(P("nonce"), 1), Has(P("nonce")))
# 0 cnf.jkt = s0, 1 cnf present, 2 a.b.c.d = s1, 3 a.b.c.d = "deep", 4 a.b.c.d has z
DEEP = (EqA(P("cnf", "jkt"), 0), Has(P("cnf")), EqA(P("a", "b", "c", "d"), 1), Eq(P("a", "b", "c", "d"), "deep"),
        Elem(P("a", "b", "c", "d"), "z"))
# 0 auth_time >= n0, 1 <= n0, 2 >= 1000, 3 <= 1000, 4 present, 5 >= n1, 6 <= n1, 7 frac present
AUTH = (GeA(P("auth_time"), 0), LeA(P("auth_time"), 0), Ge(P("auth_time"), 1000), Le(P("auth_time"), 1000),
        Has(P("auth_time")), GeA(P("auth_time"), 1), LeA(P("auth_time"), 1), Has(P("frac")))
# a numeric predicate on the exact key exp, beside the registered logic; 2 a.b.c.n >= 5, 3 a.n <= n1
EXPNUM = (Ge(P("exp"), T0), LeA(P("exp"), 0), Ge(P("a", "b", "c", "n"), 5), LeA(P("a", "n"), 1), Has(P("frac")))
# all five new ops beside the four old ones
MIXED = (EqA(P("nonce"), 0), GeA(P("auth_time"), 0), Word(P("scope"), "read"), Elem(P("roles"), "admin"),
         EqA(P("cnf", "jkt"), 1), Le(P("auth_time"), T0), Has(P("cnf")), Eq(P("nonce"), "abc"), LeA(P("auth_time"), 1),
         Ge(P("n"), -1))
PRED_SETS = collections.OrderedDict([("EMPTY", ()), ("NONCE", NONCE), ("DEEP", DEEP), ("AUTH", AUTH),
                                     ("EXPNUM", EXPNUM), ("MIXED", MIXED)])
# only the ops jg_claims_match takes: the two programs print the same
OLD_SETS = [MC.ROLES, MC.SCOPE, MC.FULL, ()]

# predicates on keys and values the corpus payloads (tests/claims_corpus.py) use; the numeric ones sit on the
# dates and on the numbers the corpus puts under x, zexp and deep/iss
CORPUS_STR = (EqA(P("sub"), 0), EqA(P("jti"), 1), EqA(P("iss"), 2), EqA(P("aud"), 3), Eq(P("x"), "y"), Has(P("x")),
              EqA(P("iss"), 0), EqA(P("sub"), 1), Elem(P("aud"), "www.example.com"))
CORPUS_NUM = (GeA(P("exp"), 0), LeA(P("exp"), 0), GeA(P("iat"), 1), Le(P("nbf"), T0), Ge(P("x"), 0), LeA(P("zexp"), 2),
              Ge(P("deep", "iss"), 1), EqA(P("sub"), 0), Has(P("exp")))
CORPUS_SETS = [CORPUS_STR, CORPUS_NUM]

D = collections.namedtuple("D", "member s0 s1 n0 n1 host", defaults=(b"", b"", 0, 0, ()))
ABC = (b"abcdefgh" * 8)
LENGTHS = (0, 1, 3, 4, 5, 63, 64)


def flip(v, k):
    """v with byte k changed to another operand byte"""
    return v[:k] + (b"A" if v[k:k + 1] != b"A" else b"B") + v[k + 1:]


@functools.lru_cache(maxsize=1)
def directed_list():
    out = []
    nonce = lambda v: b'"nonce":"' + v + b'"'
    # the operand lengths at which the window is filled 0, 1 and 2 and 16 times; s1 differs in its last byte
    for n in LENGTHS:
        v = ABC[:n]
        out.append(D(nonce(v), v, flip(v, n - 1) if n else b"x"))
    # a difference at byte 0, at bytes 3 and 4 (either side of a window boundary) and at the last byte
    for n in (5, 8, 64):
        v = ABC[:n]
        out += [D(nonce(v), flip(v, k), v) for k in sorted({0, 3, 4, n - 1})]
    # v longer or shorter than the operand by one byte
    for n in (1, 4, 5, 63):
        v = ABC[:n]
        out += [D(nonce(v + b"x"), v, v + b"x"), D(nonce(v), v + b"x", v[:-1]), D(nonce(v[:-1]), v, v[:-1])]
    out.append(D(nonce(ABC + b"x"), ABC, ABC[:63]))                    # 65 bytes against the longest operand
    # v an array, a number, null, an object, absent; v with a byte >= 0x80
    out += [D(b'"nonce":["abc"]', b"abc", b""), D(b'"nonce":123', b"123", b""), D(b'"nonce":null', b"null", b""),
            D(b'"nonce":{"nonce":"abc"}', b"abc", b"abc"), D(b'"x":"abc"', b"abc", b""), D(b'"nonce":""', b"x", b""),
            D('"nonce":"abç"'.encode(), b"ab", b"abc"), D(b'"nonce":"ab\xffc"', b"abc", b"ab"),
            D('"nonce":"çabc"'.encode(), b"abc", b"")]
    # ARG and constant EQUALS on one path, both columns equal
    out += [D(nonce(b"abc"), b"abc", b"abc"), D(nonce(b"abc"), b"abd", b"ab"), D(nonce(b"abd"), b"abd", b"abc")]
    # a repeated key whose first value equals the operand and whose last does not, and the reverse
    out += [D(b'"nonce":"n1","nonce":"n2"', b"n1", b"n2"), D(b'"nonce":"n2","nonce":"n1"', b"n1", b"n2"),
            D(b'"nonce":"n1","nonce":7', b"n1", b"n1"), D(b'"nonce":7,"nonce":"n1"', b"n1", b"n1")]
    # a nested member, a repeated parent, depth 4
    jkt = b"0ZcOCORZNYy-DWpqq30jZyJGHTN0d2HglBV3uiguA4I"
    out += [D(b'"cnf":{"jkt":"' + jkt + b'"}', jkt, b""), D(b'"cnf":{"jkt":"' + jkt + b'"}', flip(jkt, 42), b""),
            D(b'"cnf":{"jkt":"' + jkt + b'"},"cnf":{}', jkt, b""), D(b'"cnf":{},"cnf":{"jkt":"' + jkt + b'"}', jkt, b""),
            D(b'"cnf":{"jkt":"' + jkt + b'"},"cnf":{"jkt":"other"}', jkt, b""),
            D(b'"cnf":{"x":{"jkt":"' + jkt + b'"}}', jkt, b""), D(b'"jkt":"' + jkt + b'"', jkt, b""),
            D(b'"a":{"b":{"c":{"d":"deep"}}}', b"", b"deep"), D(b'"a":{"b":{"c":{"d":"deeq"}}}', b"", b"deeq"),
            D(b'"a":{"b":{"c":{"d":"deep"}}}', b"", b"dee"), D(b'"a":{"b":{"c":{"d":["z","deep"]}}}', b"", b"z"),
            D(b'"a":{"b":{"c":{"d":"deep"},"c":{}}}', b"", b"deep"),
            D(b'"cnf":{"jkt":"k"},"a":{"b":{"c":{"d":"k"}}}', b"k", b"k")]
    # numbers: 0, -0 and -1 against B = v and v +- 1
    auth = lambda lit: b'"auth_time":' + lit
    for lit, v in ((b"0", 0), (b"-0", 0), (b"-1", -1), (b"1000", 1000), (b"%d" % T0, T0)):
        out += [D(auth(lit), n0=v, n1=v + 1), D(auth(lit), n0=v - 1, n1=v), D(auth(lit), n0=v + 1, n1=v - 1)]
    big = 999999999999999
    out += [D(auth(b"%d" % big), n0=big, n1=big + 1), D(auth(b"-%d" % big), n0=-big, n1=-big - 1),
            D(auth(b"%d" % big), n0=INT64_MAX, n1=INT64_MIN), D(auth(b"-%d" % big), n0=INT64_MIN, n1=INT64_MAX),
            D(auth(b"5"), n0=(1 << 53) + 1, n1=-(1 << 53) - 1), D(auth(b"0"), n0=INT64_MIN, n1=INT64_MAX)]
    # the forms the host decides: 16 and 17 digits, fractions
    hosts = ("AUTH", "MIXED")
    out += [D(auth(b"1000000000000000"), n0=1, n1=2, host=hosts), D(auth(b"12345678901234567"), host=hosts),
            D(auth(b"-1000000000000000"), host=hosts), D(auth(b"1.0"), n0=1, n1=1, host=hosts),
            D(auth(b"0.5"), host=hosts), D(auth(b"-0.0"), host=hosts), D(auth(b"1000.000"), host=hosts)]
    # not numbers: bit 0, not HOST
    out += [D(auth(b'"123"'), n0=123, n1=123), D(auth(b"[5]"), n0=5, n1=5), D(auth(b"null")), D(auth(b"true"), n0=1),
            D(auth(b'{"auth_time":5}'), n0=5, n1=5), D(b'"x":5', n0=5, n1=5)]
    # a fraction on a path that carries only PRESENT; a fraction in an array and below another key
    out += [D(b'"frac":0.5'), D(b'"frac":0.5,"auth_time":7', n0=7, n1=8), D(b'"auth_times":0.5,"auth_tim":1.5'),
            D(b'"x":{"auth_time":0.5},"y":[0.5,{"auth_time":1.5}]')]
    # a fractional value that a later integer duplicate replaces is still the host's, and so is the reverse
    out += [D(auth(b"0.5") + b',"auth_time":5', n0=5, n1=5, host=hosts),
            D(auth(b"5") + b',"auth_time":0.5', n0=5, n1=5, host=hosts),
            D(auth(b"5") + b',"auth_time":6', n0=5, n1=6), D(auth(b"5") + b',"auth_time":"6"', n0=5, n1=5)]
    # nested numeric paths and a repeated parent
    out += [D(b'"a":{"n":3,"b":{"c":{"n":5}}}', n1=3), D(b'"a":{"n":3,"b":{"c":{"n":4}}}', n1=2),
            D(b'"a":{"b":{"c":{"n":5}}},"a":{"n":1}', n1=1), D(b'"a":{"b":{"c":{"n":5.5}}}', host=("EXPNUM",)),
            D(b'"a":{"n":2.5},"a":{"n":2}', n1=2, host=("EXPNUM",)), D(b'"a":{"b":{"n":5.5},"c":{"n":0.5}}')]
    # everything at once
    out += [D(b'"nonce":"n-0.S6_WzA2Mj","auth_time":%d,"scope":"openid read","roles":["admin"],"cnf":{"jkt":"k"},"n":-1'
              % (T0 - 30), b"n-0.S6_WzA2Mj", b"k", T0 - 60, T0),
            D(b'"nonce":"n-0.S6_WzA2Mj","auth_time":%d,"scope":"openid","roles":"admin","cnf":{"jkt":"K"},"n":-2'
              % (T0 - 90), b"n-0.S6_WzA2Mk", b"k", T0 - 60, T0 - 91),
            D(b'"nonce":"abc","auth_time":1.5,"n":0', b"abc", host=hosts),
            D(b'"nonce":"abc","auth_time":1,"n":0.5', b"abc", host=("MIXED",))]
    # the last operand of the list is not empty: packed back to back it ends at the last byte of the operand bytes
    out += [D(b'"nonce":"last"', b"x", b"last")]
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
    """The directed list's own operands: two string and two number columns"""
    dl = directed_list()
    return ([[d.s0 for d in dl], [d.s1 for d in dl]], [[d.n0 for d in dl], [d.n1 for d in dl]])


def directed_hosts(name):
    """indices of the directed cases the rule sends to the host under PRED_SETS[name]"""
    return {k for k, d in enumerate(directed_list()) if name in d.host}


def operand_ok(v):
    """what jg_claims_match_args takes as a string operand"""
    return len(v) <= _lib.PRED_VALUE_MAX and all(0x20 <= c <= 0x7e and c not in b'"\\' for c in v)


def claims_of(seg):
    try:
        m = jws._claims_map(XC.payload_of(seg))
    except Exception:
        return {}
    return m if isinstance(m, dict) else {}


def derive(cases, requires, nstr=4, nnum=4):
    """Operands for every case, from its index k alone and the value the column's first predicate reaches: the true
    value, then with its last byte changed, its first byte changed, a proper prefix, one byte more, and ""; for a
    number the value, the value +- 1, INT64_MIN, INT64_MAX and 0.  Where there is no such value: a fixed one."""
    spath, npath = {}, {}
    for path, op, value in requires:
        if op == EQUALS_ARG:
            spath.setdefault(value, path)
        if op in (NUM_GE_ARG, NUM_LE_ARG):
            npath.setdefault(value, path)
    strs, nums = [[] for _ in range(nstr)], [[] for _ in range(nnum)]
    for k, case in enumerate(cases):
        claims = claims_of(case[0])
        for c in range(nstr):
            present, v = PC.walk(claims, spath[c]) if c in spath else (False, None)
            t = v.encode() if present and isinstance(v, str) else b"none"
            if not operand_ok(t) or len(t) > 63 or not t:
                t = b"none"
            m = (k + c) % 6
            strs[c].append((t, flip(t, len(t) - 1), flip(t, 0), t[:len(t) // 2], t + b"x", b"")[m])
        for c in range(nnum):
            present, v = PC.walk(claims, npath[c]) if c in npath else (False, None)
            t = int(v) if present and isinstance(v, float) and abs(v) < 1e15 else 0
            nums[c].append((t, t + 1, t - 1, INT64_MIN, INT64_MAX, 0)[(k + c) % 6])
    return strs, nums


def value_bytes(op, value):
    if op in (EQUALS_ARG, NUM_GE_ARG, NUM_LE_ARG):
        return bytes([value])
    if op in (NUM_GE, NUM_LE):
        return struct.pack("<q", value)
    return value.encode() if isinstance(value, str) else bytes(value)


def split(requires):
    """[(path, op, value)] -> (the distinct paths in order of first use, [(path index, op, value bytes)])"""
    paths, preds = [], []
    for path, op, value in requires:
        if path not in paths:
            paths.append(path)
        preds.append((paths.index(path), op, value_bytes(op, value)))
    return tuple(paths), preds


def build_host(exe, sanitize=False):
    """Compile tests/host_unit/claims_match_args_test.cpp (claims_match_args for the CPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the scan's host model"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    src = os.path.join(ROOT, "tests", "host_unit", "claims_match_args_test.cpp")
    r = subprocess.run([cxx] + flags + ["-o", exe, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


def write_operands(path, operands):
    """(strs, nums) -> the ARGS file of the host program"""
    strs, nums = operands
    n = len(strs[0]) if strs else len(nums[0]) if nums else 0
    with open(path, "w") as f:
        f.write("A %d %d\n" % (len(strs), len(nums)))
        for k in range(n):
            f.write(" ".join(["O"] + [CC._hex(bytes(col[k])) for col in strs] + ["%d" % col[k] for col in nums]) + "\n")


def raw_args(paths, preds):
    return MC.raw_args(paths, preds)


def _run(exe, cases_path, args_path, paths, preds, env=None):
    return subprocess.run([exe, cases_path, args_path or "-"] + raw_args(paths, preds), capture_output=True, text=True,
                          timeout=300, env=env)


def run_host(exe, cases_path, args_path, requires, env=None):
    """-> (codes [int], masks [int])"""
    paths, preds = split(requires)
    r = _run(exe, cases_path, args_path, paths, preds, env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    codes, masks = [], []
    for line in r.stdout.splitlines():
        c, m = line.split()
        codes.append(int(c))
        masks.append(int(m, 16))
    return codes, masks


def rejected(exe, cases_path, args_path, paths, preds):
    """"paths" / "preds" / "args <job>" when the resolve step refuses, else None"""
    r = _run(exe, cases_path, args_path, paths, preds)
    assert r.returncode in (0, 3), (r.returncode, r.stderr[-2000:])
    words = r.stdout.split()
    assert (r.returncode == 3) == (words[:1] == ["rejected"])
    return " ".join(words[1:]) if r.returncode == 3 else None


def holds(claims, path, op, value, strs, nums):
    """One predicate on a claims map with one token's operands, as Go code on the map ValidateBatch builds decides it"""
    if op <= PRESENT:
        return MC.holds(claims, path, op, value)
    present, v = PC.walk(claims, path)
    if not present:
        return False
    if op == EQUALS_ARG:
        return isinstance(v, str) and v.encode("utf-8", "surrogatepass") == bytes(strs[value])    # Go compares bytes
    if not isinstance(v, float):                          # the oracle's numbers are float64; a bool is not one
        return False
    b = float(value if op in (NUM_GE, NUM_LE) else nums[value])
    return v >= b if op in (NUM_GE, NUM_GE_ARG) else v <= b


def evaluate(claims, requires, strs, nums):
    return sum(1 << k for k, (path, op, value) in enumerate(requires) if holds(claims, path, op, value, strs, nums))


class _Lit(str):
    """a number literal kept as its text"""


def _reached(node, path):
    """every value a scan of the text reaches along the path: through every member of a name, replaced ones too"""
    if not path:
        yield node
    elif isinstance(node, _Pairs):
        for key, v in node:
            if key == path[0]:
                yield from _reached(v, path[1:])


class _Pairs(list):
    """an object as its members in order"""


def rule_sends_to_host(payload, requires):
    """The rule of include/jg.h on the payload's text: the full path of a numeric predicate reaches a number
    literal that is not -?(0|[1-9][0-9]{0,14})"""
    doc = json.loads(payload.decode("latin-1"), object_pairs_hook=_Pairs, parse_int=_Lit, parse_float=_Lit)
    for path, op, _ in requires:
        if op not in NUMERIC:
            continue
        for v in _reached(doc, path):
            if isinstance(v, _Lit) and not DATE_FORM.fullmatch(v.encode()):
                return True
    return False


def check(cases, base_codes, codes, masks, requires, operands, hosts=None):
    """Codes: claims_extract's (base_codes), or HOST exactly where rule_sends_to_host() says so (and, with `hosts`,
    exactly at those indices).  Masks: evaluate() on the oracle's map for every non-HOST case, 0 for HOST.
    Returns (decided, extra HOST)."""
    strs, nums = operands
    assert len(cases) == len(base_codes) == len(codes) == len(masks)
    decided, extra = 0, set()
    for k, (case, base, code, mask) in enumerate(zip(cases, base_codes, codes, masks)):
        seg = case[0]
        if base == _lib.CL_HOST:
            assert code == _lib.CL_HOST and mask == 0, (k, seg, code, hex(mask))
            continue
        payload = XC.payload_of(seg)
        if rule_sends_to_host(payload, requires):
            assert code == _lib.CL_HOST and mask == 0, ("the rule sends it to the host", k, payload, code, hex(mask))
            extra.add(k)
            continue
        assert code == base, ("the code is not claims_extract's", k, payload, code, base)
        decided += 1
        s, n = [col[k] for col in strs], [col[k] for col in nums]
        want = evaluate(jws._claims_map(payload), requires, s, n)
        assert mask == want, ("mask differs from the evaluation on the oracle's map", k, payload, hex(mask), hex(want), s, n)
    if hosts is not None:
        assert extra == hosts, (sorted(extra), sorted(hosts))
    return decided, len(extra)
