"""The path-selecting claims scan (kernels/claims.hpp claims_paths_each) on the
CPU: the code k_claims_paths_each runs, built as a stand-alone program
(tests/host_unit/claims_paths_test.cpp) and run on the corpus of
tests/claims_corpus.py plus the directed list of tests/claims_paths_cases.py.

* For every path set the codes and jg_claims records are claims_extract's (the
  claims_extract_test program's), byte for byte: selecting changes no decision.
* A set of one-component paths gives the jg_selected records of the
  claims_select_test program for the same names, byte for byte.
* Every non-HOST jg_selected, cut out of the decoded payload, is the walk of the
  oracle's claims map (oracle.jws._claims_map) along each path; every HOST
  record is 80 zero bytes; nothing on the directed list is HOST.
* resolve_paths() rejects what the ABI rejects.
* The program built under ASan + UBSan prints the same output.
CPU only; nothing is loaded into Python."""
import collections
import os

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_paths_cases as PC
from tests import claims_select_cases as SC

P = PC.P


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("claims_paths")
    CC.write_cases(str(d / "cases.txt"))
    XC.write_cases(str(d / "directed.txt"), PC.directed())
    XC.write_cases(str(d / "select_directed.txt"), SC.directed() + SC.host_only())
    PC.build_host(str(d / "claims_paths_test"))
    SC.build_host(str(d / "claims_select_test"))
    XC.build_host(str(d / "claims_extract_test"))
    return d


@pytest.fixture(scope="module")
def extract_out(workdir):
    exe = str(workdir / "claims_extract_test")
    return XC.run_host(exe, str(workdir / "cases.txt")), XC.run_host(exe, str(workdir / "directed.txt"))


@pytest.fixture(scope="module")
def corpus_out(workdir):
    exe = str(workdir / "claims_paths_test")
    return {paths: PC.run_host(exe, str(workdir / "cases.txt"), paths) for paths in PC.CORPUS_SETS}


@pytest.fixture(scope="module")
def directed_out(workdir):
    exe = str(workdir / "claims_paths_test")
    return {paths: PC.run_host(exe, str(workdir / "directed.txt"), paths) for paths in PC.PATH_SETS}


def test_codes_and_records_equal_claims_extract(extract_out, corpus_out, directed_out):
    for paths, (codes, recs, _) in corpus_out.items():
        assert (codes, recs) == extract_out[0], paths
    for paths, (codes, recs, _) in directed_out.items():
        assert (codes, recs) == extract_out[1], paths
    # the existing scan decides every directed payload: HOST == 0 is a condition of the list
    assert _lib.CL_HOST not in extract_out[1][0]


def test_one_component_paths_are_claims_selects_records(workdir):
    pexe, sexe = str(workdir / "claims_paths_test"), str(workdir / "claims_select_test")
    for names, paths in zip(SC.NAME_SETS, PC.ONE_COMPONENT):
        for cases in ("select_directed.txt", "directed.txt"):
            assert PC.run_host(pexe, str(workdir / cases), paths) == SC.run_host(sexe, str(workdir / cases), names), names
    for names in ((), ("x",), SC.CORPUS_NAMES, SC.EIGHT):
        paths = tuple(P(n) for n in names)
        assert PC.run_host(pexe, str(workdir / "cases.txt"), paths) == SC.run_host(sexe, str(workdir / "cases.txt"), names)


def test_corpus_selected_are_the_oracles_walk(corpus_out):
    cases = XC.corpus_cases()
    nplain = len(CC.corpus().plain)
    for paths, (codes, _, sels) in corpus_out.items():
        assert PC.check_selected(cases[:nplain], codes[:nplain], sels[:nplain], paths, no_host=True) == nplain
        assert PC.check_selected(cases[nplain:], codes[nplain:], sels[nplain:], paths) > 200
        assert sum(1 for c, s in zip(codes, sels) if c == _lib.CL_HOST and s == bytes(80)) > 1000
    assert set(corpus_out[()][2]) == {bytes(80)}


def test_directed_list(directed_out):
    cases = PC.directed()
    payloads = PC.payloads()
    n = len(cases)
    for paths, (codes, _, sels) in directed_out.items():
        assert len(codes) == n
        assert PC.check_selected(cases, codes, sels, paths, no_host=True) == n               # HOST == 0
    assert set(directed_out[()][2]) == {bytes(80)}
    t = CC.T0 + 5
    slot = lambda paths, payload, k=0: tuple(
        SC.unpack(directed_out[paths][2][payloads.index(payload)])[f][k] for f in ("off", "len", "type"))
    absent = (0, 0, _lib.SEL_ABSENT)
    ab = PC.AB
    # the later parent replaces the earlier one wholesale
    assert slot(ab, b'{"a":{"b":1},"a":{},"exp":%d}' % t) == absent
    assert slot(ab, b'{"a":{"b":1},"a":5,"exp":%d}' % t) == absent
    assert slot(ab, b'{"a":{"b":1},"a":[{"b":2}],"exp":%d}' % t) == absent
    assert slot(ab, b'{"a":{},"a":{"b":1},"exp":%d}' % t) == (17, 1, _lib.SEL_NUMBER)
    # the last member of the name
    assert slot(ab, b'{"a":{"b":1,"b":[2]},"exp":%d}' % t) == (16, 3, _lib.SEL_ARRAY)
    # a parent that is no object; arrays are never descended
    assert slot(ab, b'{"a":null,"exp":%d}' % t) == absent
    assert slot(ab, b'{"a":[{"b":1}],"exp":%d}' % t) == absent
    # component j sits at depth j
    assert slot(ab, b'{"x":{"a":{"b":1}},"exp":%d}' % t) == absent
    assert slot(ab, b'{"b":1,"a":{"x":{"b":2}},"exp":%d}' % t) == absent
    assert slot(ab, b'{"a":{"x":{"b":2},"b":3},"exp":%d}' % t) == (22, 1, _lib.SEL_NUMBER)
    # a number ended by its parent's }, which ends the outer span too
    p = b'{"exp":%d,"a":{"b":-0.5}}' % t
    assert slot(ab, p) == (27, 4, _lib.SEL_NUMBER)
    assert slot(PC.PREFIXES, p, 0) == (22, 10, _lib.SEL_OBJECT)
    assert slot(PC.PREFIXES, p, 1) == (27, 4, _lib.SEL_NUMBER)
    # a path that is a prefix of another: the OBJECT's span and its member, down to depth 4 inside depth 6
    p = b'{"a":{"b":{"c":{"d":{"e":{"f":[]}}}}},"exp":%d}' % t
    assert [slot(PC.PREFIXES, p, k) for k in range(4)] == [
        (5, 32, _lib.SEL_OBJECT), (10, 26, _lib.SEL_OBJECT), (15, 20, _lib.SEL_OBJECT), (20, 14, _lib.SEL_OBJECT)]
    # a/b/c replaced by a later member: a/b/c/d is gone, a/b/c is the later object
    p = b'{"a":{"b":{"c":{"d":{"d":5}},"c":{"x":1}}},"exp":%d}' % t
    assert slot(PC.PREFIXES, p, 3) == absent
    assert slot(PC.PREFIXES, p, 2) == (33, 7, _lib.SEL_OBJECT)
    assert slot(PC.PREFIXES, b'{"a":{"b":{"c":{"d":true,"d":false}}}}', 3) == (29, 5, _lib.SEL_FALSE)
    # all eight slots, shared prefixes
    p = [x for x in payloads if x.startswith(b'{"realm_access":{"roles":["admin"')][0]
    assert [slot(PC.EIGHT, p, k)[2] for k in range(8)] == [
        _lib.SEL_ARRAY, _lib.SEL_ARRAY, _lib.SEL_OBJECT, _lib.SEL_STRING, _lib.SEL_ARRAY, _lib.SEL_STRING,
        _lib.SEL_ARRAY, _lib.SEL_STRING]
    p = b'{"realm_access":{"roles":"r"},"realm_access":{"groups":"g"},"exp":%d}' % t
    assert [slot(PC.EIGHT, p, k)[2] for k in range(3)] == [_lib.SEL_ABSENT, _lib.SEL_STRING, _lib.SEL_OBJECT]
    # components that are prefixes of each other
    p = [x for x in payloads if x.startswith(b'{"a":{"r":1,"roles":[2]')][0]
    assert [slot(PC.ROLE, p, k)[2] for k in range(5)] == [
        _lib.SEL_STRING, _lib.SEL_ARRAY, _lib.SEL_NUMBER, _lib.SEL_NUMBER, _lib.SEL_NULL]
    # a nested key with a byte >= 0x80 is not HOST and equals no component
    p = [x for x in payloads if x.startswith(b'{"a":{"r\xc3\xb4le":1')][0]
    assert slot(PC.ROLE, p, 0)[1:] == (1, _lib.SEL_NUMBER) and slot(PC.ROLE, p, 1) == absent
    assert slot(ab, b'{"a":{"\xff":1,"b":"after","b\xff":2},"exp":%d}' % t) == (17, 5, _lib.SEL_STRING)
    assert slot(ab, '{"a":{"b":"Jürgen"},'.encode() + b'"exp":%d}' % t) == (10, 9, _lib.SEL_STRING_RAW)
    # 64-byte components beside keys of 63 and 65 bytes
    p = [x for x in payloads if x.startswith(b'{"LLLL')][0]
    assert slot(PC.LONGS, p, 0)[1:] == (4, _lib.SEL_STRING)
    assert slot(PC.LONGS, p, 1)[1:] == (3, _lib.SEL_ARRAY)
    # every jg_sel_type at depth 2, every value start mod 3
    types = collections.Counter(t_ for s in directed_out[PC.TYPES][2] for t_ in SC.unpack(s)["type"])
    assert set(types) == set(range(9))
    for k in range(8):
        offs = {SC.unpack(s)["off"][k] % 3 for s in directed_out[PC.TYPES][2] if SC.unpack(s)["type"][k]}
        assert offs == {0, 1, 2}, k
    deep = {SC.unpack(s)["off"][3] % 3 for s in directed_out[PC.PREFIXES][2] if SC.unpack(s)["type"][3] == _lib.SEL_NUMBER}
    assert deep == {0, 1, 2}


def test_resolve_paths_rejects_what_the_abi_rejects(workdir):
    exe, cases = str(workdir / "claims_paths_test"), str(workdir / "directed.txt")
    bad = [
        [P("n%d" % k) for k in range(9)],                    # more than JG_MAX_PATHS
        [P()], [P("a"), P()],                                # no component
        [P("a", "b", "c", "d", "e")],                        # more than JG_PATH_MAX_COMP
        [P("")], [P("a", "")], [P("", "a")],                 # an empty component
        [P("a", "L" * 65)],                                  # longer than JG_SELECT_NAME_MAX
        [P("a", b"a\x1fb")], [P(b"a\x7fb")], [P("a", "b", b"a\x80b")], [P(b"\xc3\xa9", "a")], [P("a", b"a\x00b")],
        [P("a", 'a"b')], [P("a\\b", "c")],
        [P("a", "b"), P("a", "b")], [P("a"), P("b"), P("c", "d"), P("a")],     # two equal paths
        [P("a", "b", "c", "d"), P("x"), P("a", "b", "c", "d")],
    ]
    for paths in bad:
        assert PC.rejected(exe, cases, paths), paths
    good = [[], [P("a")], [P("L" * 64, "L" * 64, "L" * 64, "L" * 64)], [P(" ~", "a.b", "a/b")],
            [P("n%d" % k, "x") for k in range(8)], [P("a"), P("a", "b"), P("a", "b", "c")],
            [P("a", "b"), P("ab")], [P("ab", "c"), P("a", "bc")], [P("a", "b"), P("b", "a")], [P("a", "b"), P("a", "B")]]
    for paths in good:
        assert not PC.rejected(exe, cases, paths), paths


def test_sanitized_build_prints_the_same(workdir, corpus_out, directed_out):
    exe = str(workdir / "claims_paths_test_asan")
    PC.build_host(exe, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for paths in (PC.CORPUS_SETS[3], ()):
        assert PC.run_host(exe, str(workdir / "cases.txt"), paths, env=env) == corpus_out[paths]
    for paths in (PC.EIGHT, PC.PREFIXES, PC.ROLE, PC.LONGS):
        assert PC.run_host(exe, str(workdir / "directed.txt"), paths, env=env) == directed_out[paths]
