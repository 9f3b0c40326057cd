"""What jg_claims_match_set runs on the device, on the CPU: the claims scan with
set predicates (kernels/claims.hpp claims_match_set) against sets built by
kernels/claim_set.hpp, as a stand-alone program
(tests/host_unit/claims_match_set_test.cpp) run on the corpus of
tests/claims_corpus.py and the directed list of tests/claims_match_set_cases.py.

* Every code is claims_extract's (one numeric op's HOST rule is
  tests/claims_match_args_cases.py's); every decided mask is the plain-Python
  evaluation on the oracle's claims map (oracle.jws._claims_map) walked with
  claims_paths_cases.walk, with Python sets for the sets; every HOST mask is 0.
* Nothing on the directed list is HOST but the cases it names.
* With ops 1..11 the program prints claims_match_hash_test's output.
* The resolve step refuses what the ABI refuses.
* The program built under ASan + UBSan prints the same output.
CPU only; nothing is loaded into Python."""
import os

import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_extract_cases as XC
from tests import claims_match_args_cases as AC
from tests import claims_match_cases as MC
from tests import claims_match_hash_cases as HC
from tests import claims_match_set_cases as TC
from tests import set_model as SM

P = TC.P


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("claims_match_set")
    CC.write_cases(str(d / "cases.txt"))
    XC.write_cases(str(d / "directed.txt"), TC.directed())
    XC.write_cases(str(d / "hash_directed.txt"), HC.directed())
    HC.write_operands(str(d / "directed_args.txt"), TC.directed_operands())
    HC.write_operands(str(d / "hash_directed_args.txt"), HC.directed_operands())
    TC.write_sets(str(d / "sets.txt"), TC.sets())
    TC.write_sets(str(d / "corpus_sets.txt"), TC.corpus_sets())
    TC.build_host(str(d / "claims_match_set_test"))
    XC.build_host(str(d / "claims_extract_test"))
    return d


@pytest.fixture(scope="module")
def extract_codes(workdir):
    exe = str(workdir / "claims_extract_test")
    return XC.run_host(exe, str(workdir / "cases.txt"))[0], XC.run_host(exe, str(workdir / "directed.txt"))[0]


@pytest.fixture(scope="module")
def corpus_ops():
    cases = XC.corpus_cases()
    return {reqs: HC.derive(cases, reqs, nstr=1, nnum=0, nhash=0) for reqs in TC.CORPUS_SETS}


@pytest.fixture(scope="module")
def corpus_out(workdir, corpus_ops):
    exe, out = str(workdir / "claims_match_set_test"), {}
    for k, reqs in enumerate(TC.CORPUS_SETS):
        path = str(workdir / ("corpus_args%d.txt" % k))
        HC.write_operands(path, corpus_ops[reqs])
        out[reqs] = TC.run_host(exe, str(workdir / "cases.txt"), path, str(workdir / "corpus_sets.txt"), reqs)
    return out


@pytest.fixture(scope="module")
def directed_out(workdir):
    exe = str(workdir / "claims_match_set_test")
    return {name: TC.run_host(exe, str(workdir / "directed.txt"), str(workdir / "directed_args.txt"), str(workdir / "sets.txt"), reqs)
            for name, reqs in TC.PRED_SETS.items()}


def test_the_sets_are_what_the_list_needs():
    (s0, seed0), (s1, _), (s2, _), (s3, _) = TC.sets()
    t = SM.Table(s0, seed0)
    c = TC.collider()
    assert c not in s0 and any(SM.set_hash(c, seed0) == SM.set_hash(m, seed0) for m in s0) and t.probe(c) == (False, 1)
    a, b = SM.colliding_pairs()[1]
    assert b in s0 and a not in s0
    assert b"" in s0 and b"abc" in s0 and b"ab" not in s0 and TC.LONG in s0 and TC.LONG_OUT not in s0 and len(TC.LONG) == 255
    assert t.maxprobe >= 2 and b"jti-1" in s2 and b"jti-22" in s3 and b"jti-22" in s0


def test_directed_list(extract_codes, directed_out):
    cases, hosts = TC.directed(), TC.directed_hosts()
    assert {k for k, c in enumerate(extract_codes[1]) if c == _lib.CL_HOST} == hosts and len(hosts) == 2
    ops = TC.directed_operands()
    for name, reqs in TC.PRED_SETS.items():
        codes, masks = directed_out[name]
        decided, extra = TC.check(cases, extract_codes[1], codes, masks, reqs, ops, TC.sets(), hosts=hosts)
        assert decided == len(cases) - len(hosts) and extra == 0
        assert all(m >> len(reqs) == 0 for m in masks)
    dl, payloads, masks = TC.directed_list(), TC.payloads(), directed_out["MAIN"][1]
    exp = b',"exp":%d}' % (CC.T0 + 5)

    def bits(member, keep=0b10011111):
        ks = [k for k, d in enumerate(dl) if d.member == member]
        assert ks and payloads[ks[0]] == b"{" + member + exp, member
        return masks[ks[0]] & keep

    sid = lambda v: b'"sid":"' + v + b'"'
    # bit 0 sid in set 0, 4 sid in set 2, 7 sid is a string
    assert bits(sid(b"jti-1")) == 0b10010001 and bits(sid(b"jti-2")) == 0b10010000 and bits(sid(b"")) == 0b10000001
    assert bits(sid(b"jti-1x")) == bits(sid(b"jti-")) == bits(sid(b"ab")) == bits(sid(b"abcde")) == bits(sid(b"jti-0")) == 0b10000000
    assert bits(sid(b"abc")) == bits(sid(b"abcd")) == bits(sid(TC.LONG)) == 0b10000001
    assert bits(sid(TC.collider())) == 0b10000000 and bits(sid(SM.colliding_pairs()[0][0])) == 0b10000001
    assert bits(sid(TC.LONG + b"x")) == bits(sid(TC.LONG_OUT)) == bits(sid(TC.LONG[:254])) == bits(sid(b"jti-\xc3\xa9")) == 0b10000000
    assert bits(b'"sid":7') == bits(b'"sid":null') == bits(b'"sid":{"sid":"jti-1"}') == bits(b'"sid":[]') == 0
    assert bits(b'"sid":["jti-1"]') == 0b1000 and bits(b'"sid":[""]') == 0b1000          # ... where ELEMENT_IN_SET holds
    assert bits(sid(b"jti-1") + b"," + sid(b"nope")) == 0b10000000 and bits(sid(b"nope") + b"," + sid(b"jti-1")) == 0b10010001
    assert bits(sid(b"jti-1") + b',"sid":7') == 0 and bits(b'"sid":7,' + sid(b"jti-1")) == 0b10010001
    # bit 1 groups has an element in set 1, 2 groups is in set 1
    grp = lambda v: b'"groups":' + v
    assert bits(grp(b'"admin"')) == 0b100 and bits(grp(b"[]")) == 0 and bits(grp(b'["admin"]')) == 0b10
    assert bits(grp(b'["admin","x","y"]')) == bits(grp(b'["x","y","admin"]')) == bits(grp(b'[7,"dev",8]')) == 0b10
    assert bits(grp(b'["x",["admin"],{"k":"admin"},7,null,true,"y"]')) == 0 and bits(grp(b'[["admin"]]')) == 0
    assert bits(grp(b'["x",["zz"],{"k":"v"},7,null,false,"ops"]')) == 0b10 and bits(grp(b'["admi","admin ","dmin"]')) == 0
    assert bits(grp(b'["admin"]') + b"," + grp(b'["x"]')) == 0 and bits(grp(b'["x"]') + b"," + grp(b'["admin"]')) == 0b10
    # bits 8..11: a.b.c.d in set 0, a.b in set 0, a.b.c in set 3, a.r has an element in set 3
    deep = lambda member: bits(member, 0xf00) >> 8
    d4 = b'"a":{"b":{"c":{"d":"jti-1"}}}'
    assert deep(b'"a":"jti-1"') == 0 and deep(b'"a":{"b":"jti-1"}') == 0b0010 and deep(b'"a":{"b":{"c":"s3m"}}') == 0b0100
    assert deep(d4) == 0b0001 and deep(d4 + b',"a":{}') == 0 and deep(b'"a":{},' + d4) == 0b0001 and deep(d4 + b',"a":"abc"') == 0
    assert deep(b'"a":{"b":"jti-1"},"a":{"b":"nope"}') == 0 and deep(b'"a":{"b":"nope"},"a":{"b":"jti-1"}') == 0b0010
    assert deep(b'"a":{"r":["q","s3m"]}') == 0b1000 and deep(b'"a":{"r":"s3m"}') == 0
    # beside the older ops: bit 5 nonce = s0, 6 n >= 5
    assert bits(b'"sid":"jti-1","nonce":"n-1","n":5', 0b1110001) == 0b1110001
    assert bits(b'"sid":"jti-2","nonce":"n-1","n":4', 0b1110001) == 0b0010000
    # four sets on one path
    four = directed_out["FOUR"][1]
    at = lambda member: four[[k for k, d in enumerate(dl) if d.member == member][0]]
    assert at(sid(b"jti-1")) & 0xf == 0b0101 and at(sid(b"jti-22")) & 0xf == 0b1001 and at(sid(b"x")) & 0xf == 0b0100
    assert (at(grp(b'["jti-1","jti-2","s3m"]')) >> 4) & 0xf == 0b1101 and at(sid(b"s3m")) & 0xf == 0b1000


def test_corpus(extract_codes, corpus_out, corpus_ops):
    cases = XC.corpus_cases()
    base = extract_codes[0]
    for reqs in TC.CORPUS_SETS:
        codes, masks = corpus_out[reqs]
        decided, extra = TC.check(cases, base, codes, masks, reqs, corpus_ops[reqs], TC.corpus_sets())
        assert all(m >> len(reqs) == 0 for m in masks)
        assert decided + extra == sum(1 for b in base if b != _lib.CL_HOST) and decided > len(CC.corpus().plain)
        # the set predicates on sub, aud and iss hold on many payloads and fail on many that the scan decides
        for k in (0, 1, 3):
            hold = sum((m >> k) & 1 for m in masks)
            fail = sum(1 for c, m in zip(codes, masks) if c != _lib.CL_HOST and not (m >> k) & 1)
            assert hold >= 10 and fail >= 100, (reqs[k], hold, fail)


def test_set_ops_change_no_code(workdir, extract_codes, corpus_ops):
    exe = str(workdir / "claims_match_set_test")
    reqs = tuple(r for r in TC.CORPUS if r[1] >= TC.IN_SET)
    codes, masks = TC.run_host(exe, str(workdir / "cases.txt"), None, str(workdir / "corpus_sets.txt"), reqs)
    assert codes == extract_codes[0] and any(masks)


def test_old_ops_print_what_claims_match_hash_test_prints(workdir):
    old = str(workdir / "claims_match_hash_test")
    HC.build_host(old)
    exe = str(workdir / "claims_match_set_test")
    cases, args = str(workdir / "hash_directed.txt"), str(workdir / "hash_directed_args.txt")
    for name, reqs in HC.PRED_SETS.items():
        want = HC.run_host(old, cases, args, reqs)
        assert TC.run_host(exe, cases, args, None, reqs) == want, name
        assert TC.run_host(exe, cases, args, str(workdir / "sets.txt"), reqs) == want, name          # ... also with sets nobody asks
    ccases = XC.corpus_cases()
    for k, reqs in enumerate(HC.CORPUS_SETS):
        path = str(workdir / ("old_corpus_args%d.txt" % k))
        HC.write_operands(path, HC.derive(ccases, reqs))
        assert TC.run_host(exe, str(workdir / "cases.txt"), path, None, reqs) == HC.run_host(old, str(workdir / "cases.txt"), path, reqs)


def test_resolve_rejects_what_the_abi_rejects(workdir):
    exe, cases, args, sets = (str(workdir / n) for n in ("claims_match_set_test", "directed.txt", "directed_args.txt", "sets.txt"))
    E, H = MC.EQUALS, MC.PRESENT
    EA, IS, IN, EL = AC.EQUALS_ARG, HC.IS_STRING, TC.IN_SET, TC.ELEMENT_IN_SET
    two = (P("a"), P("b", "c"))
    bad = [
        # the ops outside 1..13
        [(0, 0, b"x")], [(0, 14, b"\0")], [(0, 255, b"\0")],
        # a set index that is not below nsets (four sets), a wrong value_len
        [(0, IN, b"\x04")], [(1, EL, b"\xff")], [(0, IN, b"")], [(0, EL, b"\0\0")],
        # two predicates of the same path, op and set
        [(0, IN, b"\0"), (1, IN, b"\0"), (0, IN, b"\0")], [(1, EL, b"\x03"), (0, H, b""), (1, EL, b"\x03")],
        # what the older entries refuse is still refused
        [(0, EA, b"\x01")], [(0, E, b"a\x80")], [(2, IN, b"\0")], [(0, HC.EQUALS_HASH, b"\0")], [(0, IS, b"x")],
        [(k % 2, IN if k < 8 else EL, bytes([k % 4])) for k in range(17)],
    ]
    for preds in bad:
        assert TC.rejected(exe, cases, args, sets, two, preds) == "preds", preds
    good = [
        [], [(0, IN, b"\0"), (0, IN, b"\x01"), (0, EL, b"\0"), (1, IN, b"\0"), (0, IS, b""), (0, EA, b"\0"), (0, H, b"")],
        [(k % 2, IN if k < 8 else EL, bytes([(k // 2) % 4])) for k in range(16)],
    ]
    for preds in good:
        assert TC.rejected(exe, cases, args, sets, two, preds) is None, preds
    # without sets every set op is refused; the older ops are not
    assert TC.rejected(exe, cases, args, None, two, [(0, IN, b"\0")]) == "preds"
    assert TC.rejected(exe, cases, args, None, two, [(0, IS, b"")]) is None
    # five sets; a set with a member the device refuses
    TC.write_sets(str(workdir / "five.txt"), [([b"m"], k) for k in range(5)])
    assert TC.rejected(exe, cases, args, str(workdir / "five.txt"), two, []) == "sets"
    for m in (b"a\x80", b'q"', b"x" * 256):
        TC.write_sets(str(workdir / "badset.txt"), [([b"ok", m], 0)])
        assert TC.rejected(exe, cases, args, str(workdir / "badset.txt"), two, []) == "sets", m
    TC.write_sets(str(workdir / "empty.txt"), [([], 0), ([b""], 0)])
    assert TC.rejected(exe, cases, args, str(workdir / "empty.txt"), two, [(0, IN, b"\0"), (0, IN, b"\x01")]) is None


def test_empty_set_matches_nothing(workdir, directed_out):
    exe = str(workdir / "claims_match_set_test")
    TC.write_sets(str(workdir / "empty.txt"), [([], 0), ([b""], 0)])
    reqs = (TC.InSet(P("sid"), 0), TC.InSet(P("sid"), 1), TC.ElemIn(P("groups"), 0))
    codes, masks = TC.run_host(exe, str(workdir / "directed.txt"), str(workdir / "directed_args.txt"), str(workdir / "empty.txt"), reqs)
    assert codes == directed_out["MAIN"][0]
    hit = [k for k, m in enumerate(masks) if m]
    assert hit and all(masks[k] == 0b10 and TC.directed_list()[k].member.endswith(b'"sid":""') for k in hit)


def test_sanitized_build_prints_the_same(workdir, corpus_out, directed_out):
    exe = str(workdir / "claims_match_set_test_asan")
    TC.build_host(exe, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for k, reqs in enumerate(TC.CORPUS_SETS):
        got = TC.run_host(exe, str(workdir / "cases.txt"), str(workdir / ("corpus_args%d.txt" % k)), str(workdir / "corpus_sets.txt"),
                          reqs, env=env)
        assert got == corpus_out[reqs]
    for name, reqs in TC.PRED_SETS.items():
        got = TC.run_host(exe, str(workdir / "directed.txt"), str(workdir / "directed_args.txt"), str(workdir / "sets.txt"), reqs, env=env)
        assert got == directed_out[name]
