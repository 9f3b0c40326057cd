"""Corpus of the registered-claims scan (kernels/claims.hpp), shared by the CPU
model test and the GPU test: payload segments, Expected sets, the oracle's
verdict for each, and the host build of the decision function.

A case is (segment bytes, index of an Expected set).  Three lists:
  plain   every case follows the scan's minimum rules: it must be decided (no
          HOST) and the code must be the oracle's string;
  hard    each case breaks one rule (or sits next to one): HOST or correct;
  random  seeded mutations of plain payloads: HOST or correct.
The oracle is oracle.jws.validate_claims(_claims_map(payload), ...) with a
passing alg header; a segment that does not decode, or a payload _claims_map
rejects, must be HOST.
"""
import base64
import functools
import json
import os
import random
import shutil
import subprocess

from cap_amd import _lib
from oracle import jws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECOND = jws.SECOND
T0 = 1611699344
B64 = set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_")
CODE_OF = {v: k for k, v in _lib.CLAIM_ERRORS.items()}

# host_cases.json tokens whose payloads are standard claim shapes
PLAIN_FIXTURES = ["claims-std", "claims-aud-string", "claims-aud-two", "claims-no-time-claims", "claims-only-exp",
                  "claims-only-iat", "claims-only-nbf", "claims-nbf-future", "claims-nbf-future-in-skew",
                  "claims-exp-past", "claims-exp-past-in-skew", "claims-iat-future", "claims-iat-null",
                  "claims-iss-null", "claims-iss-upper", "claims-jti-mixed-case", "claims-whitespace"]


def b64(payload: bytes) -> bytes:
    return base64.urlsafe_b64encode(payload).rstrip(b"=")


def js(obj) -> bytes:
    return json.dumps(obj, separators=(",", ":")).encode()


def resolve(expected: dict, now_ns: int) -> dict:
    """jwt.Expected (Go field names, durations in ns) -> the resolved form
    jg_claims_scan takes (include/jg.h): jwt/jwt.go:117-170's defaulting."""
    def leeway(d):
        s = jws._dur_seconds(d)
        return jws._f64_to_i64(0.0 if s < 0 else 150.0 if s == 0 else s)
    cks = expected.get("ClockSkewLeeway", 0)
    cks = 0 if jws._dur_seconds(cks) < 0 else 60 * SECOND if jws._dur_seconds(cks) == 0 else cks
    sec, nsec = divmod(now_ns, SECOND)
    return {"issuer": expected.get("Issuer", "").encode(), "subject": expected.get("Subject", "").encode(),
            "id": expected.get("ID", "").encode(),
            "audiences": [a.encode() for a in expected.get("Audiences") or []],
            "now_sec": sec, "now_nsec": nsec, "skew_ns": cks,
            "exp_leeway_s": leeway(expected.get("ExpirationLeeway", 0)),
            "nbf_leeway_s": leeway(expected.get("NotBeforeLeeway", 0))}


def oracle_code(seg: bytes, expected: dict, now_ns: int):
    """The jg_claim_code the host path ends in, or None when only HOST is right
    (the segment is not base64url, or the payload is no claims map)."""
    if any(c not in B64 for c in seg) or len(seg) % 4 == 1:
        return None
    payload = base64.urlsafe_b64decode(seg + b"=" * (-len(seg) % 4))
    try:
        claims = jws._claims_map(payload)
    except jws.GoJSONError:
        return None
    ex = dict(expected, SigningAlgorithms=["ES256"])
    _, err = jws.validate_claims(claims, "ES256", 1, 64, ex, now_ns)
    return CODE_OF.get(err)          # an error the scan has no code for: HOST only


class Corpus:
    def __init__(self):
        self.sets = []               # (expected dict, now_ns)
        self._index = {}
        self.plain, self.hard, self.random = [], [], []

    def set_index(self, expected, now_ns):
        key = (json.dumps(expected, sort_keys=True), now_ns)
        if key not in self._index:
            self._index[key] = len(self.sets)
            self.sets.append((expected, now_ns))
        return self._index[key]

    def add(self, where, payload, expected=None, now_ns=T0 * SECOND, raw_segment=False):
        seg = payload if raw_segment else b64(payload)
        where.append((seg, self.set_index(expected or {}, now_ns)))

    def all_cases(self):
        return self.plain + self.hard + self.random


STD = {"aud": ["www.example.com"], "exp": T0 + 600, "iat": T0, "iss": "https://example.com/", "jti": "std",
       "nbf": T0, "sub": "alice@example.com"}
FULL = {"Issuer": "https://example.com/", "Subject": "alice@example.com", "ID": "std",
        "Audiences": ["www.example.com"]}


def _nest(depth, leaf):
    """depth containers around leaf, objects and arrays alternating, every object keyed "exp"."""
    v = leaf
    for d in range(depth):
        v = {"exp": v, "iss": 5} if d % 2 == 0 else [{"aud": None, "exp": "x"}, v]
    return v


@functools.lru_cache(maxsize=1)
def corpus() -> Corpus:
    C = Corpus()
    P, H = C.plain, C.hard
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "host_cases.json")))
    fixture_sets = [dict(), dict(Issuer="https://example.com/", Audiences=["www.example.com"]),
                    dict(ClockSkewLeeway=-1 * SECOND, ExpirationLeeway=-1 * SECOND), FULL]
    for t in cases["tokens"]:
        if not t["name"].startswith("claims-"):
            continue
        seg = t["token"].split(".")[1].encode()
        payload = base64.urlsafe_b64decode(seg + b"=" * (-len(seg) % 4))
        for ex in fixture_sets:
            for d in (1, 650, -300):
                C.add(P if t["name"] in PLAIN_FIXTURES else H, payload, ex, (cases["t0"] + d) * SECOND)

    # ---------------------------------------------------------------- plain
    # every precedence pair: both checks fail, the earlier one is reported
    fails = [("none", None), ("iss", "Issuer"), ("sub", "Subject"), ("jti", "ID"), ("aud", "Audiences"),
             ("nbf", None), ("exp", None), ("iat", None)]
    for a in range(len(fails)):
        for b in range(a + 1, len(fails)):
            claims, ex = dict(STD), dict(FULL)
            for name, field in (fails[a], fails[b]):
                if name == "none":
                    for k in ("exp", "nbf", "iat"):
                        claims.pop(k)
                elif field == "Audiences":
                    ex[field] = ["other"]
                elif field:
                    ex[field] = "other"
                elif name == "nbf":
                    claims["nbf"] = T0 + 1000
                elif name == "exp":
                    claims["exp"] = T0 - 1000
                elif name == "iat":
                    claims["iat"] = T0 + 1000
            if fails[a][0] == "none" and fails[b][1] is None:
                continue                      # no time claims at all: a time failure cannot be set up beside it
            C.add(P, js(claims), ex)
    # exp / nbf / iat: every subset of {absent, null, 0, present}
    for e in ("absent", None, 0, T0 + 600):
        for n in ("absent", None, 0, T0 - 10):
            for i in ("absent", None, 0, T0 - 20):
                claims = {k: v for k, v in (("exp", e), ("nbf", n), ("iat", i)) if v != "absent"}
                for ex in ({}, {"ExpirationLeeway": 5 * SECOND, "NotBeforeLeeway": 7 * SECOND},
                           {"ExpirationLeeway": -SECOND, "NotBeforeLeeway": -SECOND}):
                    C.add(P, js(claims), ex)
                    C.add(P, js(claims), ex, (T0 + 100) * SECOND)
    # negative and 15-digit dates
    for claims in ({"exp": -5}, {"nbf": -1, "exp": 999999999999999}, {"iat": -999999999999999},
                   {"exp": 999999999999999}, {"nbf": 999999999999999}, {"iat": 100000000000000, "exp": 1},
                   {"exp": -999999999999999, "nbf": -999999999999999}):
        for now in (T0 * SECOND, -5 * SECOND, 999999999999999 * SECOND // 1000000, -(1 << 62), (1 << 63) - 1):
            C.add(P, js(claims), {}, now)
            C.add(P, js(claims), {"ClockSkewLeeway": (1 << 63) - 1}, now)
    # now on each window edge +-1 ns, with default / zero-meaning-default / negative leeways
    for skew, cks in ((0, 60 * SECOND), (-1, 0), (1500000000, 1500000000), (1, 1)):
        ex = {"ClockSkewLeeway": skew}
        for d in (-1, 0, 1):
            C.add(P, js({"nbf": T0, "exp": T0 + 10 ** 6}), ex, T0 * SECOND - cks + d)        # now + skew == nbf
            C.add(P, js({"iat": T0, "exp": T0 + 10 ** 6}), ex, T0 * SECOND - cks + d)        # now + skew == iat
            C.add(P, js({"exp": T0, "nbf": T0 - 10 ** 6}), ex, T0 * SECOND + cks + d)        # now - skew == exp
            C.add(P, js({"exp": T0, "nbf": T0 - 10 ** 6}), ex, T0 * SECOND + cks + d - SECOND)
            for lw in (0, -SECOND, 30 * SECOND, 1500000000):
                ex2 = dict(ex, ExpirationLeeway=lw, NotBeforeLeeway=lw)
                el = 150 if lw == 0 else max(0, lw // SECOND)
                C.add(P, js({"iat": T0}), ex2, (T0 + el) * SECOND + cks + d)                   # defaulted exp edge
                C.add(P, js({"exp": T0}), ex2, (T0 - el) * SECOND - cks + d)                   # defaulted nbf edge
    # aud shapes x expected audiences (1, 2, 16; hit in the first / last place)
    sixteen = ["aud-%02d" % k for k in range(16)]
    for aud in ("www.example.com", [], ["www.example.com"], ["x", "y", "www.example.com"], ["www.example.com", "x"],
                ["aud-15"], ["q", "aud-00"], "", [""], ["www.example.co"], ["www.example.com."]):
        for exp_aud in (["www.example.com"], ["nope", "www.example.com"], ["www.example.com", "nope"], sixteen,
                        sixteen[:15] + ["www.example.com"], [""], []):
            C.add(P, js(dict(STD, aud=aud)), {"Audiences": exp_aud})
    C.add(P, js({k: v for k, v in STD.items() if k != "aud"}), {"Audiences": ["www.example.com"]})
    # an expected string longer than the claim, and a prefix of it
    for field, key in (("Issuer", "iss"), ("Subject", "sub"), ("ID", "jti")):
        for want in (STD[key] + "x", STD[key][:-1], STD[key], "x" + STD[key][1:], STD[key].upper()):
            C.add(P, js(STD), {field: want})
        C.add(P, js({k: v for k, v in STD.items() if k != key}), {field: STD[key]})
        C.add(P, js(dict(STD, **{key: ""})), {field: STD[key]})
        C.add(P, js(dict(STD, **{key: None})), {field: STD[key]})
    # nesting to depth 32 with keys named exp; whitespace; key casing
    for depth in (1, 2, 5, 31):
        C.add(P, js(dict(STD, deep=_nest(depth, "leaf"))), FULL)
        C.add(P, js({"deep": _nest(depth, 7), "exp": T0 - 1000}), {})
        C.add(P, js({"exp": T0 + 5, "deep": _nest(depth - 1, [])}), {})
    C.add(P, b' \t\r\n{ \t\r\n"exp" \t\r\n: \t\r\n%d \t\r\n, \t\r\n"aud" \t\r\n: \t\r\n[ \t\r\n"a" \t\r\n, \t\r\n"b" \t\r\n]'
          b' \t\r\n, \t\r\n"o" \t\r\n: \t\r\n{ \t\r\n} \t\r\n, "a":[ \r\n] } \t\r\n' % (T0 + 5), {"Audiences": ["b"]})
    for keys in (("ISS", "SUB", "JTI", "AUD", "EXP", "NBF", "IAT"), ("Iss", "sUb", "jtI", "AuD", "eXP", "NbF", "IaT")):
        claims = {k2: STD[k.lower()] for k, k2 in zip(keys, keys)}
        C.add(P, js(claims), FULL)
        C.add(P, js(claims), dict(FULL, Issuer="other"))
        C.add(P, js(dict(claims, **{keys[4]: T0 - 1000})), FULL)
    # other members of every type, non-ASCII text and DEL inside strings that are no claim values
    C.add(P, js(dict(STD, a=True, b=False, c=None, d=-0.5, e=[1.25, "x", [], {}], f={"issuer": "x"}, isss="y", i="z")),
          FULL)
    C.add(P, ('{"exp":%d,"name":"Jürgen 中 \x7f","o":{"kéy":"vé"},"n":-0,"z":0.0,"big":12345678901234567}'
              % (T0 + 5)).encode(), {})
    for pad in range(0, 7):                    # every segment length mod 4, every tail shape
        C.add(P, js({"exp": T0 + 5, "p": "x" * pad}), {})

    # ---------------------------------------------------------------- hard
    std = js(STD)
    # duplicates and case-variant duplicates
    H_ = lambda payload, ex=None, now=T0 * SECOND: C.add(H, payload, ex, now)
    H_(b'{"exp":1,"exp":%d}' % (T0 + 5))
    H_(b'{"exp":%d,"exp":1}' % (T0 + 5))
    H_(b'{"exp":%d,"EXP":1}' % (T0 + 5))
    H_(b'{"Exp":1,"eXp":%d}' % (T0 + 5))
    H_(b'{"exp":%d,"iss":"a","ISS":"https://example.com/"}' % (T0 + 5), FULL)
    H_(b'{"exp":%d,"aud":"a","Aud":["www.example.com"]}' % (T0 + 5), FULL)
    H_(b'{"exp":%d,"x":1,"x":2}' % (T0 + 5))
    # long-s and Kelvin-sign keys (fold to sub / ... under Go's matching)
    H_(('{"exp":%d,"ſub":"alice@example.com"}' % (T0 + 5)).encode(), {"Subject": "alice@example.com"})
    H_(('{"exp":%d,"sub":"x","ſub":"alice@example.com"}' % (T0 + 5)).encode(), {"Subject": "alice@example.com"})
    H_(('{"exp":%d,"K":"v","iſſ":"https://example.com/"}' % (T0 + 5)).encode(), FULL)
    H_(('{"exp":%d,"kéy":1}' % (T0 + 5)).encode())
    # escapes in keys, in claim values and in other values
    H_(b'{"e\\u0078p":%d}' % (T0 - 1000))
    H_(b'{"exp":%d,"iss":"https:\\/\\/example.com\\/"}' % (T0 + 5), FULL)
    H_(b'{"exp":%d,"aud":["www.example.com\\u0000"]}' % (T0 + 5), FULL)
    H_(b'{"exp":%d,"other":"a\\nb"}' % (T0 + 5))
    H_(b'{"exp":%d,"other":"a\\qb"}' % (T0 + 5))
    H_(b'{"exp":%d,"other":"a\\"}' % (T0 + 5))
    H_(b'{"exp":%d,"o":{"k\\u0041":1}}' % (T0 + 5))
    # bytes >= 0x80 in claim values
    H_(('{"exp":%d,"iss":"https://exämple.com/"}' % (T0 + 5)).encode(), {"Issuer": "https://exämple.com/"})
    H_(b'{"exp":%d,"iss":"a\xff\xfeb"}' % (T0 + 5), {"Issuer": "a��b"})
    H_(('{"exp":%d,"aud":["é"]}' % (T0 + 5)).encode(), {"Audiences": ["é"]})
    H_(('{"exp":%d,"aud":"é"}' % (T0 + 5)).encode(), {"Audiences": ["é"]})
    H_(('{"exp":%d,"sub":"é","jti":"é"}' % (T0 + 5)).encode())
    # numbers
    for num in (b"1e999", b"-0", b"1.5", b"1234567890123456", b"9" * 400, b"1E3", b"1e3", b"01", b"-", b"1.", b".5",
                b"-a", b"+1", b"0x10", b"1.5e3", b"0.0", b"-1.0", b"00", b"1-", b"999999999999999", b"1000000000000000",
                b"-999999999999999", b"123456789012345678", b"0.1234567890123456", b"-0.0", b"1.e1", b"Infinity", b"NaN"):
        H_(b'{"exp":' + num + b'}')
        H_(b'{"nbf":' + num + b',"exp":%d}' % (T0 + 5))
        H_(b'{"exp":%d,"x":' % (T0 + 5) + num + b'}')
        H_(b'{"exp":%d,"x":[' % (T0 + 5) + num + b']}')
    # control bytes
    for c in (0, 1, 0x1f, 0x0a, 0x09, 0x0b, 0x0c, 0x7f, 0x80, 0xa0, 0xff):
        H_(b'{"exp":%d,"x":"a' % (T0 + 5) + bytes([c]) + b'b"}')
        H_(b'{"exp":%d,"x' % (T0 + 5) + bytes([c]) + b'":1}')
        H_(b'{"exp":%d,"iss":"a' % (T0 + 5) + bytes([c]) + b'b"}')
        H_(b'{"exp":%d' % (T0 + 5) + bytes([c]) + b',"x":1}')
        H_(bytes([c]) + b'{"exp":%d}' % (T0 + 5))
        H_(b'{"exp":%d}' % (T0 + 5) + bytes([c]))
    # truncation at every byte of one payload
    full = js(dict(STD, extra={"k": [1, 2.5, None, True, False]}, s="t"))
    for cut in range(len(full)):
        H_(full[:cut], FULL)
    # trailing garbage, depth 33, null, [1], the empty segment, literals
    for tail in (b"x", b"{}", b",", b"}", b"]", b"null", b"\x00", b" 1"):
        H_(std + tail, FULL)
    for depth in (32, 33, 34, 64, 200):
        H_(js({"exp": T0 - 1000, "deep": _nest(depth, 1)}))
        H_(b'{"exp":%d,"d":' % (T0 + 5) + b"[" * depth + b"]" * depth + b"}")
    for doc in (b"null", b"[1]", b"", b" ", b"1", b'"s"', b"true", b"{", b"}", b"{}", b"[]", b"{}{}", b"{} {}", b"nul",
                b'{"exp":tru}', b'{"exp":%d,"x":nul}' % T0, b'{"exp":%d,"x":nulll}' % T0, b'{"exp":%d,"x":True}' % T0,
                b'{"exp":%d,"x":falsey}' % T0, b'{"exp":%d,"x":t}' % T0, b'{"exp":%d,}' % T0, b'{,"exp":%d}' % T0,
                b'{"exp":%d,"a":[1,]}' % T0, b'{"exp":%d,"a":[,1]}' % T0, b'{"exp" %d}' % T0, b'{"exp"::%d}' % T0,
                b'{exp:%d}' % T0, b"{'exp':%d}" % T0, b'{"exp":%d "x":1}' % T0, b'{"exp":%d,"a":[1 2]}' % T0,
                b'{"exp":%d,"a":[1}' % T0, b'{"exp":%d,"a":{"b":1]}' % T0, b'{"exp":%d]' % T0, b'{"a":1,"exp":%d}}' % T0,
                b'{"exp":%d,"a":"unterminated}' % T0, b'{"exp":%d,"a":[1]]}' % T0, b'\xef\xbb\xbf{"exp":%d}' % T0,
                b'{"exp":%d}\x0c' % T0, b'{"exp":%d,"":1}' % (T0 + 5), b'{"":{"":[]},"exp":%d}' % (T0 + 5)):
        H_(doc)
    # base64: a bad byte, length % 4 == 1, nonzero trailing bits, padding
    good = b64(b'{"exp":%d,"p":"x"}' % (T0 + 5))
    assert len(good) % 4 == 3
    for pos in (0, 1, 2, 3, 4, len(good) // 2, len(good) - 2, len(good) - 1):
        for bad in (b"+", b"/", b"=", b".", b" ", b"\n", b"\x00", b"\x80", b"\xff", b"@", b"[", b"`", b"{"):
            C.add(H, good[:pos] + bad + good[pos + 1:], {}, raw_segment=True)
    C.add(H, good + b"A", {}, raw_segment=True)              # well-formed JSON plus a 0x00... decodes differently
    C.add(H, good + b"AA", {}, raw_segment=True)             # length % 4 == 1
    C.add(H, good[:-2], {}, raw_segment=True)                # length % 4 == 1
    C.add(H, b"A", {}, raw_segment=True)
    C.add(H, b"e", {}, raw_segment=True)
    C.add(H, good + b"=", {}, raw_segment=True)
    for payload in (b'{"exp":%d} ' % (T0 + 5), b'{"exp":%d}  ' % (T0 + 5)):
        seg = b64(payload)
        assert len(seg) % 4 in (2, 3)
        alphabet = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
        last = alphabet.index(seg[-1:])
        for extra in range(1, 16 if len(seg) % 4 == 2 else 4):
            C.add(H, seg[:-1] + alphabet[last + extra:last + extra + 1], {}, raw_segment=True)   # unused bits set
    # the type mismatches
    others = [b"1", b"-1.5", b"true", b"false", b"null", b'"s"', b"[]", b'["s"]', b"{}", b'{"a":1}', b"[1]", b"[null]",
              b'[["s"]]', b'["s",1]', b'["s",null]', b'["s",["t"]]', b'["s",{}]', b'[true]', b'""']
    for key in (b"iss", b"sub", b"jti", b"aud", b"exp", b"nbf", b"iat", b"AUD", b"Exp"):
        for v in others:
            tail = b"nbf" if key == b"iat" else b"iat"
            H_(b'{"zexp":1,"' + key + b'":' + v + b',"' + tail + b'":%d}' % T0, FULL)
    # ---------------------------------------------------------------- random
    rng = random.Random(20261019)
    seeds = [s for s, _ in P if len(s) > 8]
    alphabet = b'{}[]":,0123456789.-+eE\\ \t\n\r\x00\x7f\x80\xc3\xa9tfnulasxpibjd'
    rsets = [({}, T0 * SECOND), (FULL, T0 * SECOND), (dict(FULL, Issuer="other"), (T0 + 700) * SECOND),
             ({"Audiences": ["b", "www.example.com"], "ClockSkewLeeway": -1}, (T0 - 700) * SECOND)]
    for k in range(4000):
        seg = rng.choice(seeds)
        payload = bytearray(base64.urlsafe_b64decode(seg + b"=" * (-len(seg) % 4)))
        for _ in range(rng.choice((1, 1, 1, 2, 3))):
            op = rng.randrange(6)
            at = rng.randrange(len(payload) + 1)
            if op == 0 and payload:
                del payload[min(at, len(payload) - 1)]
            elif op == 1:
                payload.insert(at, rng.choice(alphabet))
            elif op == 2 and payload:
                payload[min(at, len(payload) - 1)] = rng.choice(alphabet)
            elif op == 3 and payload:
                a2 = rng.randrange(len(payload) + 1)
                lo, hi = min(at, a2), min(max(at, a2), min(at, a2) + 24)
                payload[at:at] = payload[lo:hi]                  # duplicate a slice (duplicate keys, nesting)
            elif op == 4 and payload:
                i = min(at, len(payload) - 1)
                payload[i] = payload[i] ^ (1 << rng.randrange(8))
            else:
                payload[at:at] = rng.choice((b'"exp":1,', b'"ISS":"x",', b'"aud":[', b"null", b"{", b"}", b'"nbf":0,'))
        ex, now = rng.choice(rsets)
        if rng.randrange(10) == 0:                               # mutate the segment itself
            seg = bytearray(b64(bytes(payload)))
            if seg:
                seg[rng.randrange(len(seg))] = rng.choice(b"AB+/=_-.Zz09 ")
            C.add(C.random, bytes(seg), ex, now, raw_segment=True)
        else:
            C.add(C.random, bytes(payload), ex, now)
    return C


@functools.lru_cache(maxsize=1)
def oracle_codes():
    """oracle_code of every case of the corpus, in all_cases() order (computed once)."""
    C = corpus()
    return [oracle_code(seg, *C.sets[si]) for seg, si in C.all_cases()]


def _hex(b: bytes) -> str:
    return b.hex() if b else "-"


def write_cases(path):
    C = corpus()
    with open(path, "w") as f:
        for ex, now_ns in C.sets:
            r = resolve(ex, now_ns)
            f.write("E %s %s %s %d %s%d %d %d %d %d\n" % (
                _hex(r["issuer"]), _hex(r["subject"]), _hex(r["id"]), len(r["audiences"]),
                "".join(_hex(a) + " " for a in r["audiences"]), r["now_sec"], r["now_nsec"], r["skew_ns"],
                r["exp_leeway_s"], r["nbf_leeway_s"]))
        for seg, si in C.all_cases():
            f.write("C %d %s\n" % (si, _hex(seg)))


def build_host(exe, sanitize=False):
    """Compile tests/host_unit/claims_scan_test.cpp (kernels/claims.hpp for the CPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the scan's host model"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host_unit", "claims_scan_test.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def run_host(exe, cases_path, env=None):
    r = subprocess.run([exe, cases_path], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    return [int(x) for x in r.stdout.split()]


def check(codes, where="all"):
    """Every code is HOST or the oracle's; on the plain list none is HOST.  Returns the HOST count."""
    C = corpus()
    want = oracle_codes()
    cases = C.all_cases()
    assert len(codes) == len(cases)
    nplain = len(C.plain)
    host = 0
    for k, ((seg, si), got, w) in enumerate(zip(cases, codes, want)):
        if got == _lib.CL_HOST:
            assert k >= nplain, ("plain case left to the host", k, seg, C.sets[si])
            host += 1
            continue
        assert 0 <= got < _lib.CL_HOST and got == w, ("scan code differs from the oracle", k, got, w, seg, C.sets[si])
    return host
