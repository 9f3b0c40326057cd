"""match_requires (host/cap_jwt.cpp), the one function MatchBatch's host path
evaluates its requirements with, against the plain-Python evaluation on the
oracle's claims map: every predicate set of tests/claims_match_cases.py on every
directed payload, and some the scan would not take.  CPU only."""
import pytest

from oracle import jws
from tests import claims_match_cases as MC

H = pytest.importorskip("cap_amd._capjwt_host")
P = MC.P


def native(reqs):
    return [(list(p), op, val) for p, op, val in reqs]


def test_directed_payloads_under_every_predicate_set():
    n = 0
    for reqs in MC.PRED_SETS[1:]:
        for payload in MC.payloads():
            assert H.match_requires(payload, native(reqs)) == MC.evaluate(jws._claims_map(payload), reqs), (payload, reqs)
            n += 1
    assert n > 1000
    assert H.match_requires(b'{"a":1}', []) == 0


def test_requirements_the_scan_does_not_take():
    payload = ('{"scope":"a  b\\u0020c","rôles":["rôle","x y"],"deep":{"a":{"b":{"c":{"d":{"e":null}}}}},'
               '"long":"' + "v" * 70 + '","q":"say \\"hi\\""}').encode()
    reqs = (MC.Word(P("scope"), ""), MC.Word(P("scope"), "c"), MC.Word(P("scope"), "a  b"), MC.Eq(P("scope"), "a  b c"),
            MC.Elem(P("rôles"), "rôle"), MC.Elem(P("rôles"), "x y"), MC.Word(P("rôles"), "x"),
            MC.Has(P("deep", "a", "b", "c", "d", "e")), MC.Has(P("deep", "a", "b", "c", "d", "e", "f")),
            MC.Eq(P("long"), "v" * 70), MC.Eq(P("long"), "v" * 69), MC.Eq(P("q"), 'say "hi"'), MC.Elem(P("q"), ""),
            MC.Has(P("")), MC.Eq(P("scope"), "a  b c"), MC.Has(P("scope", "x")))
    assert len(reqs) == 16
    want = MC.evaluate(jws._claims_map(payload), reqs)
    assert H.match_requires(payload, native(reqs)) == want == 0b0100_1010_1011_1011


def test_what_every_path_refuses():
    for reqs in ([(["a"], 4, "")] * 17, [([], 4, "")], [(["a"], 1, "x\0y")], [(["a", "b\0"], 4, "")], [(["a"], 0, "")],
                 [(["a"], 5, "")]):
        with pytest.raises(ValueError):
            H.match_requires(b"{}", reqs)
