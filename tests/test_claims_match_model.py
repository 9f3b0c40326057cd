"""The predicate-matching claims scan (kernels/claims.hpp claims_match_each) on
the CPU: the code k_claims_match_each runs, built as a stand-alone program
(tests/host_unit/claims_match_test.cpp) and run on the corpus of
tests/claims_corpus.py plus the directed list of tests/claims_match_cases.py.

* For every predicate set the codes are claims_extract's (the
  claims_extract_test program's): predicates change no decision, so the decided
  share is that test's.
* Every non-HOST mask is the plain-Python evaluation of the predicates on the
  oracle's claims map (oracle.jws._claims_map, walked with
  claims_paths_cases.walk); every HOST mask is 0; nothing on the directed list
  is HOST.
* resolve_preds() rejects what the ABI rejects.
* The program built under ASan + UBSan prints the same output.
CPU only; nothing is loaded into Python."""
import os

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_match_cases as MC

P = MC.P
Eq, Word, Elem, Has = MC.Eq, MC.Word, MC.Elem, MC.Has


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("claims_match")
    CC.write_cases(str(d / "cases.txt"))
    XC.write_cases(str(d / "directed.txt"), MC.directed())
    MC.build_host(str(d / "claims_match_test"))
    XC.build_host(str(d / "claims_extract_test"))
    return d


@pytest.fixture(scope="module")
def extract_codes(workdir):
    exe = str(workdir / "claims_extract_test")
    return XC.run_host(exe, str(workdir / "cases.txt"))[0], XC.run_host(exe, str(workdir / "directed.txt"))[0]


@pytest.fixture(scope="module")
def corpus_out(workdir):
    exe = str(workdir / "claims_match_test")
    return {reqs: MC.run_host(exe, str(workdir / "cases.txt"), reqs) for reqs in MC.CORPUS_SETS}


@pytest.fixture(scope="module")
def directed_out(workdir):
    exe = str(workdir / "claims_match_test")
    return {reqs: MC.run_host(exe, str(workdir / "directed.txt"), reqs) for reqs in MC.PRED_SETS}


def test_codes_equal_claims_extract(extract_codes, corpus_out, directed_out):
    for reqs, (codes, _) in corpus_out.items():
        assert codes == extract_codes[0], reqs
    for reqs, (codes, _) in directed_out.items():
        assert codes == extract_codes[1], reqs
    # the existing scan decides every directed payload: HOST == 0 is a condition of the list
    assert _lib.CL_HOST not in extract_codes[1]
    # ... and one of them with a failure code, whose mask is filled all the same
    assert _lib.CL_EXP in extract_codes[1] and _lib.CL_NBF in extract_codes[1]


def test_corpus_masks_are_the_evaluation_on_the_oracles_map(corpus_out):
    cases = XC.corpus_cases()
    nplain = len(CC.corpus().plain)
    for reqs, (codes, masks) in corpus_out.items():
        assert MC.check_masks(cases[:nplain], codes[:nplain], masks[:nplain], reqs, no_host=True) == nplain
        assert MC.check_masks(cases[nplain:], codes[nplain:], masks[nplain:], reqs) > 200
        assert sum(1 for c, m in zip(codes, masks) if c == _lib.CL_HOST and m == 0) > 1000
        assert all(m >> len(reqs) == 0 for m in masks)
    assert set(corpus_out[()][1]) == {0}
    # the sets are not idle on the corpus: several predicates hold on many payloads
    for reqs in MC.CORPUS_SETS[1:]:
        hit = sum(1 for k in range(len(reqs)) if any((m >> k) & 1 for m in corpus_out[reqs][1]))
        assert hit >= 5 and sum(bin(m).count("1") for m in corpus_out[reqs][1]) > 1000, (reqs, hit)


def test_directed_list(directed_out):
    cases = MC.directed()
    payloads = MC.payloads()
    n = len(cases)
    for reqs, (codes, masks) in directed_out.items():
        assert len(codes) == n
        assert MC.check_masks(cases, codes, masks, reqs, no_host=True) == n                 # HOST == 0
        assert all(m >> len(reqs) == 0 for m in masks)
    assert set(directed_out[()][1]) == {0}
    exp = b',"exp":%d}' % (CC.T0 + 5)

    def bits(reqs, member):
        return directed_out[reqs][1][payloads.index(b"{" + member + exp)]
    R, A, S, L, D = MC.ROLES, MC.AR, MC.SCOPE, MC.LONGV, MC.DEEP
    # ROLES: 0 has admin, 1 has user, 2 present, 3 equals admin, 4 has word admin.  The last member wins
    assert bits(R, b'"roles":["admin"],"roles":["user"]') == 0b00110
    assert bits(R, b'"roles":["user"],"roles":["admin"]') == 0b00101
    assert bits(R, b'"roles":["admin"],"roles":"admin"') == 0b11100
    assert bits(R, b'"roles":"admin","roles":null') == 0b00100
    assert bits(R, b'"x":{"roles":["admin"]}') == 0
    # AR: 0 a/r has x, 1 a/r present, 2 a present, 3 a/r equals x.  A repeated parent replaces the earlier one
    assert bits(A, b'"a":{"r":["x"]},"a":{}') == 0b0100
    assert bits(A, b'"a":{"r":["x"]},"a":5') == 0b0100
    assert bits(A, b'"a":{},"a":{"r":["x"]}') == 0b0111
    assert bits(A, b'"a":{"r":["x"]},"a":[{"r":["x"]}]') == 0b0100
    assert bits(A, b'"a":null') == 0b0100 and bits(A, b'"a":{"r":null}') == 0b0110 and bits(A, b'"b":1') == 0
    # prefixes and suffixes
    assert bits(R, b'"roles":["administrator","adm","xadmin","admiN"]') == 0b00100
    assert bits(R, b'"roles":["administrator","adm","xadmin","admiN","admin"]') == 0b00101
    for v in (b"administrator", b"adm", b"xadmin", b"admiN"):
        assert bits(R, b'"roles":"' + v + b'"') == 0b00100
    # SCOPE: 0 word read, 1 word read:all, 2 = read, 3 = "", 4 = "read write", 5 present, 6 element read,
    # 7 word write, 8 = " read"
    assert bits(S, b'"scope":"read:all"') == 0b000100010
    assert bits(S, b'"scope":"thread"') == 0b000100000
    assert bits(S, b'"scope":"write read"') == 0b010100001
    assert bits(S, b'"scope":"read:all read"') == 0b000100011           # two values with one prefix, in one pass
    assert bits(S, b'"scope":"read read:all"') == 0b000100011
    assert bits(S, b'"scope":" read"') == 0b100100001
    assert bits(S, b'"scope":"read "') == 0b000100001
    assert bits(S, b'"scope":"a  read"') == 0b000100001
    assert bits(S, b'"scope":""') == 0b000101000
    assert bits(S, b'"scope":"read"') == 0b000100101
    assert bits(S, b'"scope":"read write"') == 0b010110001
    assert bits(S, '"scope":"réad read"'.encode()) == 0b000100001
    assert bits(S, '"scope":"réad"'.encode()) == 0b000100000
    assert bits(S, b'"scope":"re\xffad write"') == 0b010100000
    assert bits(S, b'"scope":"read\xc2\xa0write"') == 0b000100000       # U+00A0 separates nothing
    assert bits(S, b'"scope":["read"]') == 0b001100000
    assert bits(S, b'"scope":null') == 0b000100000
    # elements: only strings, only direct ones, and the depth is restored after a nested container closes
    for v in (b"[]", b"[1,null,true,false,-2.5]", b'[["admin"]]', b'[{"admin":"admin"}]',
              b'[{"roles":["admin"]},["admin",["admin"]]]', b'["admin user"]', '["admín"]'.encode()):
        assert bits(R, b'"roles":' + v) == 0b00100, v
    for v in (b'["x",["y"],"admin"]', b'["x",{"k":["z"]},"admin"]', '["admín","admin"]'.encode(), b'["",1,"admin"]'):
        assert bits(R, b'"roles":' + v) == 0b00101, v
    assert bits(R, b'"roles":"admin"') == 0b11100
    # LONGV: 0 = V64, 1 element V64, 2 word V64, 3 = V64[:63]
    v = MC.V64.encode()
    assert bits(L, b'"k":"' + v + b'"') == 0b0101
    assert bits(L, b'"k":"' + v + b'v"') == 0
    assert bits(L, b'"k":"' + v[:63] + b'"') == 0b1000
    assert bits(L, b'"k":["' + v + b'v","' + v + b'"]') == 0b0010
    assert bits(L, b'"k":"x ' + v + b'"') == 0b0100
    # DEEP: 0 a/b/c/d has z, 1 it is present, 2 a/b/c is present, 3 a/b/c/d = z, 4 = deep
    assert bits(D, b'"a":{"b":{"c":{"d":["y","z"]}}}') == 0b00111
    assert bits(D, b'"a":{"b":{"c":{"d":"z"}}}') == 0b01110
    assert bits(D, b'"a":{"b":{"c":{"d":[{"d":["z"]}]}}}') == 0b00110
    assert bits(D, b'"a":{"b":{"c":{"d":["z"]},"c":{}}}') == 0b00100
    assert bits(D, b'"a":{"b":{"c":{"d":["y",["z"],{"d":"z"},"z"]}}}') == 0b00111
    # registered names as paths: 0 aud has www, 1 aud = www, 2 sub = alice, 3 sub word alice, 4 exp present, 5 aud has b
    G = directed_out[MC.REGISTERED][1]
    tail = b',"exp":%d}' % (CC.T0 + 5)
    assert G[payloads.index(b'{"aud":"www.example.com","sub":"alice@example.com"' + tail)] == 0b011110
    assert G[payloads.index(b'{"aud":["b","www.example.com"],"sub":"alice@example.com"' + tail)] == 0b111101
    # a failure code with a filled mask
    k = payloads.index(b'{"roles":["admin"],"scope":"read","exp":%d}' % (CC.T0 - 86400))
    assert directed_out[R][0][k] == _lib.CL_EXP and directed_out[R][1][k] == 0b00101
    assert directed_out[S][1][k] == 0b000100101
    # an enclosing object with PRESENT and its member with HAS_ELEMENT; all sixteen predicates over eight paths
    k = [i for i, x in enumerate(payloads) if x.startswith(b'{"realm_access":{"roles":["admin","dev"')][0]
    assert directed_out[MC.ENCLOSING][1][k] == 0b11111
    assert directed_out[MC.FULL][1][k] == 0b0111_1011_0111_1111
    k = payloads.index(b'{"realm_access":{"roles":"r"},"realm_access":{"groups":"g"},"exp":%d}' % (CC.T0 + 5))
    assert directed_out[MC.ENCLOSING][1][k] == 0b00001


def test_resolve_preds_rejects_what_the_abi_rejects(workdir):
    exe, cases = str(workdir / "claims_match_test"), str(workdir / "directed.txt")
    E, W, L, H = MC.EQUALS, MC.HAS_WORD, MC.HAS_ELEMENT, MC.PRESENT
    two = (P("a"), P("b", "c"))
    bad = [
        [(k % 2, L, b"v%d" % k) for k in range(17)],                           # more than JG_MAX_PRED
        [(2, E, b"x")], [(0, E, b"x"), (255, H, b"")],                         # a path index past the paths
        [(0, 0, b"x")], [(0, 5, b"")], [(0, 255, b"x")],                       # an unknown op
        [(0, E, b"v" * 65)], [(0, W, b"")], [(0, W, b"v" * 65)], [(0, L, b"")], [(0, L, b"v" * 65)], [(0, H, b"x")],
        [(0, E, b"a\x1fb")], [(0, E, b"a\x7fb")], [(1, L, b"a\x80b")], [(0, L, b"\xc3\xa9")], [(0, E, b"a\x00b")],
        [(0, E, b'a"b')], [(1, W, b"a\\b")],
        [(0, W, b"a b")], [(0, W, b" ")],                                      # a space in a HAS_WORD value
        [(0, E, b"x"), (0, E, b"x")], [(1, H, b""), (0, H, b""), (1, H, b"")], [(0, E, b""), (1, E, b"x"), (0, E, b"")],
        [(0, L, b"abc"), (0, W, b"abc"), (1, L, b"abc"), (0, L, b"abc")],      # two identical predicates
    ]
    for preds in bad:
        assert MC.rejected(exe, cases, two, preds) == "preds", preds
    assert MC.rejected(exe, cases, (), [(0, H, b"")]) == "preds"              # no path to name
    # what jg_claims_paths refuses is refused here
    for paths in ([P("n%d" % k) for k in range(9)], [P()], [P("a", "b", "c", "d", "e")], [P("")], [P("a"), P("a")],
                  [P('a"b')]):
        assert MC.rejected(exe, cases, paths, []) == "paths", paths
    good = [
        [], [(0, E, b"")], [(0, E, b"a b"), (0, E, b" ")], [(0, E, b"v" * 64), (0, W, b"v" * 64), (0, L, b"v" * 64)],
        [(0, E, b"x"), (1, E, b"x"), (0, L, b"x"), (0, W, b"x")], [(0, E, b"x"), (0, E, b"X"), (0, E, b"xx")],
        [(0, H, b""), (1, H, b"")], [(k % 2, L, b"v%d" % k) for k in range(16)], [(1, L, b" ~"), (1, E, b"a.b/c")],
    ]
    for preds in good:
        assert MC.rejected(exe, cases, two, preds) is None, preds


def test_sanitized_build_prints_the_same(workdir, corpus_out, directed_out):
    exe = str(workdir / "claims_match_test_asan")
    MC.build_host(exe, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for reqs in (MC.CORPUS_SETS[2], ()):
        assert MC.run_host(exe, str(workdir / "cases.txt"), reqs, env=env) == corpus_out[reqs]
    for reqs in (MC.FULL, MC.SCOPE, MC.ROLES, MC.LONGV, MC.DEEP):
        assert MC.run_host(exe, str(workdir / "directed.txt"), reqs, env=env) == directed_out[reqs]
