"""The selecting claims scan (kernels/claims.hpp claims_select) on the CPU: the
code k_claims_select runs, built as a stand-alone program
(tests/host_unit/claims_select_test.cpp) and run on the corpus of
tests/claims_corpus.py plus the directed list of tests/claims_select_cases.py.

* For every name set the codes and jg_claims records are claims_extract's (the
  claims_extract_test program's), byte for byte: selecting changes no decision.
* Every non-HOST jg_selected, cut out of the decoded payload, is the oracle's
  claims-map entry (oracle.jws._claims_map) per name; every HOST record is 80
  zero bytes; nothing on the directed list is HOST; with no names every record
  is zero.
* resolve_select() rejects what the ABI rejects.
* The program built under ASan + UBSan prints the same output.
CPU only; nothing is loaded into Python."""
import collections
import os

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_select_cases as SC

CORPUS_NAMES = SC.CORPUS_NAMES
CORPUS_SETS = [(), ("x",), CORPUS_NAMES, SC.EIGHT]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("claims_select")
    CC.write_cases(str(d / "cases.txt"))
    XC.write_cases(str(d / "directed.txt"), SC.directed() + SC.host_only())
    SC.build_host(str(d / "claims_select_test"))
    XC.build_host(str(d / "claims_extract_test"))
    return d


@pytest.fixture(scope="module")
def extract_out(workdir):
    exe = str(workdir / "claims_extract_test")
    return XC.run_host(exe, str(workdir / "cases.txt")), XC.run_host(exe, str(workdir / "directed.txt"))


@pytest.fixture(scope="module")
def corpus_out(workdir):
    exe = str(workdir / "claims_select_test")
    return {names: SC.run_host(exe, str(workdir / "cases.txt"), names) for names in CORPUS_SETS}


@pytest.fixture(scope="module")
def directed_out(workdir):
    exe = str(workdir / "claims_select_test")
    return {names: SC.run_host(exe, str(workdir / "directed.txt"), names) for names in SC.NAME_SETS}


def test_codes_and_records_equal_claims_extract(extract_out, corpus_out, directed_out):
    for names, (codes, recs, _) in corpus_out.items():
        assert (codes, recs) == extract_out[0], names
    for names, (codes, recs, _) in directed_out.items():
        assert (codes, recs) == extract_out[1], names


def test_corpus_selected_are_the_oracles_map_entries(corpus_out):
    cases = XC.corpus_cases()
    nplain = len(CC.corpus().plain)
    for names, (codes, _, sels) in corpus_out.items():
        assert SC.check_selected(cases[:nplain], codes[:nplain], sels[:nplain], names, no_host=True) == nplain
        assert SC.check_selected(cases[nplain:], codes[nplain:], sels[nplain:], names) > 200
        assert sum(1 for c, s in zip(codes, sels) if c == _lib.CL_HOST and s == bytes(80)) > 1000
    types = collections.Counter(t for s in corpus_out[CORPUS_NAMES][2] for t in SC.unpack(s)["type"])
    assert set(types) == set(range(9))                       # the corpus alone reaches every jg_sel_type
    # a failure code carries a filled record too
    codes, _, sels = corpus_out[CORPUS_NAMES]
    filled = {c for c, s in zip(codes, sels) if s != bytes(80)}
    assert filled == set(range(_lib.CL_HOST))


def test_no_names_every_record_is_zero(corpus_out, directed_out):
    assert set(corpus_out[()][2]) == {bytes(80)}
    assert set(directed_out[()][2]) == {bytes(80)}


def test_directed_list(directed_out):
    cases = SC.directed()
    payloads = SC.payloads()
    n = len(cases)
    for names, (codes, _, sels) in directed_out.items():
        assert len(codes) == n + 1
        assert SC.check_selected(cases, codes[:n], sels[:n], names, no_host=True) == n     # HOST == 0
        assert codes[n] == _lib.CL_HOST and sels[n] == bytes(80)                            # the 18-byte number
    t = CC.T0 + 5
    slot = lambda names, payload, k=0: tuple(
        SC.unpack(directed_out[names][2][payloads.index(payload)])[f][k] for f in ("off", "len", "type"))
    one = ("scope",)
    # "": the position after the opening quote, length 0
    assert slot(one, b'{"scope":"","exp":%d}' % t) == (10, 0, _lib.SEL_STRING)
    assert slot(one, b'{"scope":[],"exp":%d}' % t) == (9, 2, _lib.SEL_ARRAY)
    assert slot(one, b'{"scope":{},"exp":%d}' % t) == (9, 2, _lib.SEL_OBJECT)
    assert slot(one, b'{"scope":-0,"exp":%d}' % t) == (9, 2, _lib.SEL_NUMBER)
    assert slot(one, b'{"scope":12345678901234567,"exp":%d}' % t) == (9, 17, _lib.SEL_NUMBER)
    assert slot(one, b'{"scope":null,"exp":%d}' % t) == (9, 4, _lib.SEL_NULL)               # NULL, not ABSENT
    assert slot(one, b'{"exp":%d,"scope":1.5}' % t) == (26, 3, _lib.SEL_NUMBER)             # ended by the last }
    # STRING_RAW takes the quotes in
    assert slot(one, b'{"scope":"a\xffb","exp":%d}' % t) == (9, 5, _lib.SEL_STRING_RAW)
    # depth 2 never matches and does not disturb the outer span
    assert slot(one, b'{"o":{"scope":"inner","x":{"scope":2}},"scope":"outer","exp":%d}' % t) == (48, 5, _lib.SEL_STRING)
    assert slot(one, b'{"o":[{"scope":[1]}],"exp":%d}' % t) == (0, 0, _lib.SEL_ABSENT)
    assert slot(one, b'{"scope":{"scope":"inner"},"exp":%d}' % t) == (9, 17, _lib.SEL_OBJECT)
    # twice at depth 1: the last wins, type and all
    assert slot(one, b'{"scope":"first","scope":[1,2],"exp":%d}' % t) == (25, 5, _lib.SEL_ARRAY)
    assert slot(one, b'{"scope":{"a":1},"scope":null,"exp":%d}' % t) == (25, 4, _lib.SEL_NULL)
    assert slot(one, b'{"scope":"a long first value","scope":""}') == (39, 0, _lib.SEL_STRING)
    # prefixes of each other
    pre = ("scope", "scopes", "s")
    p = b'{"s":1,"scopes":[2],"scope":"three","sc":4,"scopex":5,"exp":%d}' % t
    assert [slot(pre, p, k)[2] for k in range(3)] == [_lib.SEL_STRING, _lib.SEL_ARRAY, _lib.SEL_NUMBER]
    p = b'{"scopes":"only the longer one","exp":%d}' % t
    assert [slot(pre, p, k)[2] for k in range(3)] == [_lib.SEL_ABSENT, _lib.SEL_STRING, _lib.SEL_ABSENT]
    # case-sensitive
    assert slot(("Scope",), b'{"scope":"x","exp":%d}' % t)[2] == _lib.SEL_ABSENT
    assert slot(("Scope",), b'{"Scope":"upper","scope":"lower","exp":%d}' % t) == (10, 5, _lib.SEL_STRING)
    # a registered name: ABSENT in the slot under another casing, still read by the registered logic
    p = b'{"SUB":"alice@example.com","exp":%d}' % t
    assert slot(("sub", "scope"), p)[2] == _lib.SEL_ABSENT
    rec = directed_out[("sub", "scope")][1][payloads.index(p)]
    assert XC.claims_of_record(cases[payloads.index(p)][0], rec)["sub"] == "alice@example.com"
    assert slot(("sub", "scope"), b'{"sub":"bob","exp":%d}' % t) == (8, 3, _lib.SEL_STRING)
    # 1 byte and 64 bytes beside keys of 63 and 65
    p = [x for x in payloads if x.startswith(b'{"k":1,"LLLL')][0]
    assert slot(("k", SC.LONG), p, 0) == (5, 1, _lib.SEL_NUMBER)
    assert slot(("k", SC.LONG), p, 1) == (75, 4, _lib.SEL_STRING)
    # all eight present
    p = [x for x in payloads if x.startswith(b'{"scope":"a b","roles"')][0]
    assert [slot(SC.EIGHT, p, k)[2] for k in range(8)] == [
        _lib.SEL_STRING, _lib.SEL_ARRAY, _lib.SEL_OBJECT, _lib.SEL_STRING, _lib.SEL_STRING, _lib.SEL_NULL,
        _lib.SEL_NUMBER, _lib.SEL_STRING]
    # every value start mod 3
    assert {SC.unpack(s)["off"][0] % 3 for s in directed_out[one][2] if SC.unpack(s)["type"][0]} == {0, 1, 2}


def test_resolve_select_rejects_what_the_abi_rejects(workdir):
    exe, cases = str(workdir / "claims_select_test"), str(workdir / "directed.txt")
    bad = [
        ["n%d" % k for k in range(9)],                       # more than JG_MAX_SELECT
        [""], ["scope", ""],                                 # an empty name
        ["L" * 65],                                          # longer than JG_SELECT_NAME_MAX
        [b"a\x1fb"], [b"a\x7fb"], [b"a\x80b"], [b"\xc3\xa9"], [b"a\x00b"],
        ['a"b'], ["a\\b"],
        ["scope", "scope"], ["a", "b", "c", "a"],            # two equal names
    ]
    for names in bad:
        assert SC.rejected(exe, cases, names), names
    good = [[], ["a"], ["L" * 64], [" ~"], ["n%d" % k for k in range(8)], ["scope", "Scope"], ["a", "ab", "abc"]]
    for names in good:
        assert not SC.rejected(exe, cases, names), names


def test_sanitized_build_prints_the_same(workdir, corpus_out, directed_out):
    exe = str(workdir / "claims_select_test_asan")
    SC.build_host(exe, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for names in (CORPUS_NAMES, ()):
        assert SC.run_host(exe, str(workdir / "cases.txt"), names, env=env) == corpus_out[names]
    for names in (SC.EIGHT, ("scope", "scopes", "s"), ("k", SC.LONG)):
        assert SC.run_host(exe, str(workdir / "directed.txt"), names, env=env) == directed_out[names]
