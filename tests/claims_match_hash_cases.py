"""Shared by the tests of the claims scan with hash columns (hash_operand /
k_hash_operand / IS_STRING in claims_match_args / jg_claims_match_hash): the two
new predicate forms, the value a hash claim must equal, the directed list with
its operands and sources, the derivation of sources for the corpus, the host
build of tests/host_unit/claims_match_hash_test.cpp, and the plain-Python
evaluation on the oracle's claims map.

A predicate is (path, op, value) as in tests/claims_match_args_cases.py; for
EQUALS_HASH the value is the hash column (an int), for IS_STRING it is "".
Operands are a triple (strs, nums, hashes): lists of columns, each with one entry
per case; a hash column's entry is (source bytes, fam) or None for "no value"
(fam 0).

A directed case is D(member, s0, h0, h1): the payload {member,"exp":..} with its
own operand for one string column and its sources for two hash columns.
claims_extract alone decides every directed payload.
"""
import base64
import collections
import functools
import hashlib
import os
import shutil
import subprocess

from cap_amd import _lib
from oracle import jws
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_match_args_cases as AC
from tests import claims_match_cases as MC
from tests import claims_paths_cases as PC

ROOT = CC.ROOT
T0 = CC.T0
P = PC.P
EQUALS_HASH, IS_STRING = 10, 11                                          # jg_pred_op (include/jg.h)
SHA256, SHA384, SHA512 = 1, 2, 3                                         # jg_hash_fam
FAMS = (SHA256, SHA384, SHA512)
HASHLIB = {SHA256: hashlib.sha256, SHA384: hashlib.sha384, SHA512: hashlib.sha512}
NCHAR = {SHA256: 22, SHA384: 32, SHA512: 43}
# the source lengths at which SHA-256 (55 / 56, 119 / 120) and SHA-512 (111 / 112, 239 / 240) take one block more,
# the block sizes themselves +- 1, and the cap
LENGTHS = (0, 1, 54, 55, 56, 63, 64, 65, 111, 112, 119, 120, 127, 128, 129, 239, 240, 8191, 8192)

Eq, Has, EqA, Ge = MC.Eq, MC.Has, AC.EqA, AC.Ge
EqH = lambda path, col: (path, EQUALS_HASH, col)
IsStr = lambda path: (path, IS_STRING, "")


def hash_value(src, fam):
    """What at_hash / c_hash must equal (oidc/id_token.go verifyHashClaim): bytes"""
    d = HASHLIB[fam](bytes(src)).digest()
    return base64.urlsafe_b64encode(d[:len(d) // 2]).rstrip(b"=")


def source(k, n):
    """n bytes that depend on k: any byte values, as an access token is any string"""
    return hashlib.shake_128(b"src-%d" % k).digest(n)


# 0 at_hash is a string, 1 = hash column 0, 2 c_hash is a string, 3 = hash column 1, 4 nonce = s0, 5 at_hash present,
# 6.. the depths: a.b.c.d is a string, = hash column 0, a.b / a.b.c / a are strings
HS = (IsStr(P("at_hash")), EqH(P("at_hash"), 0), IsStr(P("c_hash")), EqH(P("c_hash"), 1), EqA(P("nonce"), 0),
      Has(P("at_hash")), IsStr(P("a", "b", "c", "d")), EqH(P("a", "b", "c", "d"), 0), IsStr(P("a", "b")),
      IsStr(P("a", "b", "c")), IsStr(P("a")))
# the new ops alone; the same column under two paths; both columns on one path
ONLY = (IsStr(P("at_hash")), EqH(P("at_hash"), 0), EqH(P("c_hash"), 0), EqH(P("at_hash"), 1))
PRED_SETS = collections.OrderedDict([("HS", HS), ("ONLY", ONLY)])

# on keys and values the corpus payloads (tests/claims_corpus.py) use, a numeric op among them: its HOST rule holds on
CORPUS = (IsStr(P("sub")), IsStr(P("aud")), IsStr(P("exp")), IsStr(P("x")), EqH(P("sub"), 0), EqA(P("sub"), 0),
          IsStr(P("deep", "iss")), Has(P("x")), EqH(P("jti"), 1), Ge(P("exp"), T0), IsStr(P("iss")), IsStr(P("deep")))
CORPUS_SETS = [CORPUS]

D = collections.namedtuple("D", "member s0 h0 h1", defaults=(b"", None, None))


@functools.lru_cache(maxsize=1)
def directed_list():
    out = []
    at = lambda v: b'"at_hash":"' + v + b'"'
    both = lambda a, c: at(a) + b',"c_hash":"' + c + b'","nonce":"n-1"'
    tok, code = b"ya29.a0AfH6SMBx-access-token", b"SplxlOBeZQQYbYS6WxSbIA"
    # every family, right on both columns; then the source wrong in its first or last byte
    for fam in FAMS:
        a, c = hash_value(tok, fam), hash_value(code, fam)
        out += [D(both(a, c), b"n-1", (tok, fam), (code, fam)),
                D(both(a, c), b"n-2", (AC.flip(tok, 0), fam), (AC.flip(code, len(code) - 1), fam)),
                D(both(a, c), b"n-1", (tok, fam), None), D(both(a, c), b"n-1", None, (code, fam)),
                D(both(c, a), b"n-1", (tok, fam), (code, fam))]                      # the claims swapped
        # the family of another alg: the value has another length, or the same length and other bytes
        out += [D(both(a, c), b"n-1", (tok, other), (code, other)) for other in FAMS if other != fam]
    # sources at the block boundaries of both hashes, the empty source
    for k, n in enumerate((0, 1, 55, 56, 64, 111, 112, 128, 240)):
        src, fam = source(k, n), FAMS[k % 3]
        out += [D(at(hash_value(src, fam)), b"", (src, fam), (src, FAMS[(k + 1) % 3]))]
    a = hash_value(tok, SHA256)
    # one character more, one less, the last one changed; a byte >= 0x80
    out += [D(at(a + b"A"), b"", (tok, SHA256)), D(at(a[:-1]), b"", (tok, SHA256)), D(at(AC.flip(a, 21)), b"", (tok, SHA256)),
            D(at(AC.flip(a, 0)), b"", (tok, SHA256)), D(at(a[:8] + b"\xc3\xa7" + a[10:]), b"", (tok, SHA256)),
            D(at(a[:21] + b"\xff"), b"", (tok, SHA256))]
    # not a string: "", a number, null, a literal, an array that holds the value, an object, absent
    for v in (b'""', b"123", b"-0.5", b"null", b"true", b'["' + a + b'"]', b'{"at_hash":"' + a + b'"}', b"[]", b"{}"):
        out += [D(b'"at_hash":' + v, b"", (tok, SHA256), (tok, SHA256))]
    out += [D(b'"x":"' + a + b'"', b"", (tok, SHA256), (tok, SHA256))]
    # no value for the job (fam 0): a string is still a string and never equal, "" and a one-byte string included
    out += [D(at(a), b"", None, None), D(at(b""), b"", None, None), D(at(b"A"), b"", None, None), D(at(b" "), b"", None)]
    # a key named twice: the last member wins, in both orders, for both ops
    wrong = hash_value(b"other", SHA256)
    out += [D(at(a) + b',"at_hash":7', b"", (tok, SHA256)), D(b'"at_hash":7,' + at(a), b"", (tok, SHA256)),
            D(at(a) + b"," + at(wrong), b"", (tok, SHA256)), D(at(wrong) + b"," + at(a), b"", (tok, SHA256)),
            D(at(a) + b',"at_hash":null', b"", (tok, SHA256)), D(b'"at_hash":[],' + at(b""), b"", (tok, SHA256)),
            D(at(a) + b',"at_hash":{"at_hash":"' + a + b'"}', b"", (tok, SHA256))]
    # depths 1..4 and a repeated parent
    deep = lambda leaf: b'"a":{"b":{"c":{"d":' + leaf + b"}}}"
    q = b'"' + a + b'"'
    out += [D(b'"a":"s"'), D(b'"a":{"b":"s"}'), D(b'"a":{"b":{"c":"s"}}'), D(deep(q), b"", (tok, SHA256)),
            D(deep(b"5"), b"", (tok, SHA256)), D(deep(q) + b',"a":{}', b"", (tok, SHA256)),
            D(b'"a":{},' + deep(q), b"", (tok, SHA256)), D(deep(q) + b',"a":"s"', b"", (tok, SHA256)),
            D(b'"a":{"b":{"c":{"d":' + q + b'},"c":"s"}}', b"", (tok, SHA256)),
            D(b'"a":{"b":{"c":"s","c":{"d":' + q + b"}}}", b"", (tok, SHA256)),
            D(b'"a":{"b":"s","b":{"c":{"d":""}}}', b"", (tok, SHA256)), D(b'"a":{"b":[{"c":"s"}]}')]
    # the last source of the list is not empty: packed back to back it ends at the last byte of the source bytes
    out += [D(both(a, hash_value(code, SHA512)), b"n-1", (tok, SHA256), (code, SHA512))]
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
    """The directed list's own operands: one string column, no number, two hash columns"""
    dl = directed_list()
    return ([[d.s0 for d in dl]], [], [[d.h0 for d in dl], [d.h1 for d in dl]])


def derive(cases, requires, nstr=2, nnum=1, nhash=2):
    """Operands for every case: AC.derive()'s strings and numbers, and sources from the index alone, of every
    family and none, of lengths 0..200"""
    strs, nums = AC.derive(cases, requires, nstr=nstr, nnum=nnum)
    hashes = [[None if (k + c) % 4 == 3 else (source(k + 1000 * c, (37 * k + c) % 201), FAMS[(k + c) % 4])
               for k in range(len(cases))] for c in range(nhash)]
    return strs, nums, hashes


def value_bytes(op, value):
    if op == EQUALS_HASH:
        return bytes([value])
    if op == IS_STRING:
        return b""
    return AC.value_bytes(op, value)


def split(requires):
    """[(path, op, value)] -> (the distinct paths in order of first use, [(path index, op, value bytes)])"""
    paths, preds = [], []
    for path, op, value in requires:
        if path not in paths:
            paths.append(path)
        preds.append((paths.index(path), op, value_bytes(op, value)))
    return tuple(paths), preds


def build_host(exe, sanitize=False):
    """Compile tests/host_unit/claims_match_hash_test.cpp (the scan and hash_operand for the CPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the scan's host model"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "host_kernels")]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    src = os.path.join(ROOT, "tests", "host_unit", "claims_match_hash_test.cpp")
    r = subprocess.run([cxx] + flags + ["-o", exe, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


def write_operands(path, operands):
    """(strs, nums, hashes) -> the ARGS file of the host program"""
    strs, nums, hashes = operands
    n = len(strs[0]) if strs else len(nums[0]) if nums else len(hashes[0]) if hashes else 0
    src = lambda h: "0:-" if h is None else "%d:%s" % (h[1], CC._hex(bytes(h[0])))
    with open(path, "w") as f:
        f.write("A %d %d %d\n" % (len(strs), len(nums), len(hashes)))
        for k in range(n):
            f.write(" ".join(["O"] + [CC._hex(bytes(col[k])) for col in strs] + ["%d" % col[k] for col in nums] +
                             [src(col[k]) for col in hashes]) + "\n")


def _run(exe, cases_path, args_path, paths, preds, env=None):
    return subprocess.run([exe, cases_path, args_path or "-"] + MC.raw_args(paths, preds), capture_output=True, text=True,
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
    """"paths" / "preds" / "args <job>" / "hsrc <job>" when the resolve step refuses, else None"""
    r = _run(exe, cases_path, args_path, paths, preds)
    assert r.returncode in (0, 3), (r.returncode, r.stderr[-2000:])
    words = r.stdout.split()
    assert (r.returncode == 3) == (words[:1] == ["rejected"])
    return " ".join(words[1:]) if r.returncode == 3 else None


def run_operands(exe, rows, workdir, env=None):
    """rows: (fam, offset, source) -> the operand the host build of hash_operand() makes for each: [bytes]"""
    path = os.path.join(str(workdir), "operands.txt")
    with open(path, "w") as f:
        for fam, off, src in rows:
            f.write("%d %d %s\n" % (fam, off, CC._hex(bytes(src))))
    r = subprocess.run([exe, "--operands", path], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    out = []
    for line in r.stdout.splitlines():
        n, _, hx = line.partition(" ")
        v = bytes.fromhex(hx)
        assert len(v) == int(n)
        out.append(v)
    assert len(out) == len(rows)
    return out


def holds(claims, path, op, value, strs, nums, hs):
    """One predicate on a claims map with one token's operands and sources, as Go code on the map decides it"""
    if op < EQUALS_HASH:
        return AC.holds(claims, path, op, value, strs, nums)
    present, v = PC.walk(claims, path)
    if not present or not isinstance(v, str):
        return False
    if op == IS_STRING:
        return True
    return hs[value] is not None and v.encode("utf-8", "surrogatepass") == hash_value(*hs[value])


def evaluate(claims, requires, strs, nums, hs):
    return sum(1 << k for k, (path, op, value) in enumerate(requires) if holds(claims, path, op, value, strs, nums, hs))


def check(cases, base_codes, codes, masks, requires, operands):
    """Codes: claims_extract's (base_codes), or HOST exactly where AC.rule_sends_to_host() says so: the new ops change
    no code.  Masks: evaluate() on the oracle's map for every non-HOST case, 0 for HOST.  Returns (decided, extra HOST)."""
    strs, nums, hashes = operands
    assert len(cases) == len(base_codes) == len(codes) == len(masks)
    decided = extra = 0
    for k, (case, base, code, mask) in enumerate(zip(cases, base_codes, codes, masks)):
        seg = case[0]
        if base == _lib.CL_HOST:
            assert code == _lib.CL_HOST and mask == 0, (k, seg, code, hex(mask))
            continue
        payload = XC.payload_of(seg)
        if AC.rule_sends_to_host(payload, requires):
            assert code == _lib.CL_HOST and mask == 0, ("the rule sends it to the host", k, payload, code, hex(mask))
            extra += 1
            continue
        assert code == base, ("the code is not claims_extract's", k, payload, code, base)
        decided += 1
        s, n, h = [col[k] for col in strs], [col[k] for col in nums], [col[k] for col in hashes]
        want = evaluate(jws._claims_map(payload), requires, s, n, h)
        assert mask == want, ("mask differs from the evaluation on the oracle's map", k, payload, hex(mask), hex(want), s, h)
    return decided, extra
