"""Adding to a resident set, without a GPU:

- tests/set_add_model.py's checker refuses every single mistake a kernel could
  make, applied to a correct result: a member twice, a member dropped, a wrong
  hash, a hole in a chain, maxprobe one too small, an old slot moved, a pool
  prefix byte changed, n off by one, a ref into the middle of an entry;
- the insertion and the rehash step of kernels/claim_set_insert.hpp, compiled
  for the CPU with a sequential compare-and-swap
  (tests/host_unit/claim_set_add_test.cpp), pass the checker on the directed
  adds, and set_probe on the result equals Python's `in`;
- the same program built with ASan + UBSan prints the same.
"""
import pytest

from tests import set_add_model as AM
from tests import set_model as SM


@pytest.fixture(scope="module")
def good():
    """A correct add without growth that has a chain: three residents and two added members of one home slot"""
    same = SM._with_home(9, 64, 5)
    resident = same[:3] + [b"id-%d" % k for k in range(17)]
    added = [b"new-%d" % k for k in range(6)] + same[3:]
    t = SM.Table(resident, SM.SEED)
    assert t.nslots == 64
    slots, pool, nslots, maxprobe, n, cnt = AM.set_add(t.slots, t.pool, t.n, t.maxprobe, SM.SEED, added)
    assert (nslots, n, cnt) == (64, 28, 8) and maxprobe >= 5
    r = dict(slots=slots, pool=pool, nslots=nslots, maxprobe=maxprobe, n=n, old_slots=list(t.slots), old_pool=list(t.pool),
             members=resident + added, last=same[4], resident_last=same[2])
    check(r)
    return r


def check(r, **over):
    a = dict(r, **over)
    AM.check_added(a["slots"], a["pool"], a["nslots"], a["maxprobe"], a["n"], SM.SEED, a["old_slots"], a["old_pool"], a["members"])


def slot_of(r, m):
    ent = AM.entries(r["pool"])
    return next(i for i, (h, ref) in enumerate(r["slots"]) if ref and ent[ref - 1] == m)


def first_empty_from(slots, i):
    while slots[i % len(slots)][1]:
        i += 1
    return i % len(slots)


def test_reference_add_is_legal_and_grows_as_the_runtime_does():
    assert [AM.grown_nslots(*a) for a in ((1, 0, 1), (16, 5, 3), (16, 8, 1), (16, 8, 56), (16, 8, 57), (64, 3, 0))] == \
        [2, 16, 32, 128, 256, 64]
    for name, resident, added in AM.directed_adds():
        t = SM.Table(resident, SM.SEED)
        slots, pool, nslots, maxprobe, n, cnt = AM.set_add(t.slots, t.pool, t.n, t.maxprobe, SM.SEED, added)
        union = list(dict.fromkeys(resident + added))
        AM.check_added(slots, pool, nslots, maxprobe, n, SM.SEED, t.slots, t.pool, union, old_maxprobe=t.maxprobe)
        assert cnt == len(union) - t.n and n == len(union), name
        assert len(pool) == len(t.pool) + sum(len(AM.pack_entry(m)) for m in added), name
        for q in AM.queries_for(resident, added):
            assert AM.contains(slots, pool, nslots, maxprobe, SM.SEED, q) == (q in set(union)), (name, q)


def test_directed_adds_are_what_they_are_named_for():
    D = {name: (SM.Table(resident, SM.SEED), resident, added) for name, resident, added in AM.directed_adds()}
    grown = lambda name: AM.grown_nslots(D[name][0].nslots, D[name][0].n, len(D[name][2]))
    assert (D["to-the-empty-set"][0].nslots, grown("to-the-empty-set")) == (1, 2)
    assert (D["fill-to-half"][0].nslots, grown("fill-to-half")) == (16, 16) and D["fill-to-half"][0].n + 3 == 8
    assert (D["one-more-doubles"][0].nslots, grown("one-more-doubles")) == (16, 32)
    assert (D["three-doublings"][0].nslots, grown("three-doublings")) == (16, 128)
    assert set(D["all-resident"][2]) <= set(D["all-resident"][1]) and grown("all-resident") == 16
    assert set(D["all-resident-grows"][2]) == set(D["all-resident-grows"][1]) and grown("all-resident-grows") == 32
    assert len(D["one-string-64-times"][2]) == 64 == len(D["64-of-one-home-grows"][2])
    assert grown("one-string-64-times") == 512 == D["one-string-64-times"][0].nslots and grown("one-string-64-times-grows") == 256
    assert grown("28-of-one-home") == 256 == D["28-of-one-home"][0].nslots
    t, resident, added = D["64-of-one-home-grows"]
    assert grown("64-of-one-home-grows") == 256 and {SM.set_hash(m, SM.SEED) & 255 for m in added} == {5} and len(set(added)) == 64
    t, resident, added = D["same-state-pairs"]
    assert all(SM.hash_state(a) == SM.hash_state(b) for a, b in zip(resident[:6], added))
    t, resident, added = D["wraps"]
    slots, pool, nslots, maxprobe, n, cnt = AM.set_add(t.slots, t.pool, t.n, t.maxprobe, SM.SEED, added)
    i = next(i for i, (h, ref) in enumerate(slots) if ref and (h, ref) not in t.slots)
    assert nslots == 8 and slots[i][0] & 7 == 7 and i < 7 and cnt == 1              # home 7, lies past the last slot


def test_checker_refuses_a_member_twice(good):
    s = list(good["slots"])
    i = slot_of(good, good["last"])
    s[first_empty_from(s, i)] = s[i]
    with pytest.raises(AssertionError, match="two slots"):
        check(good, slots=s, n=good["n"] + 1)


def test_checker_refuses_a_member_dropped(good):
    s = list(good["slots"])
    s[slot_of(good, good["last"])] = (0, 0)
    with pytest.raises(AssertionError, match="members differ"):
        check(good, slots=s, n=good["n"] - 1)


def test_checker_refuses_a_wrong_hash(good):
    s = list(good["slots"])
    i = slot_of(good, good["last"])
    s[i] = (s[i][0] ^ 0x10000, s[i][1])                                            # same home slot, another hash
    with pytest.raises(AssertionError, match="hash"):
        check(good, slots=s)


def test_checker_refuses_a_hole_in_a_chain(good):
    s = list(good["slots"])
    i = slot_of(good, good["last"])
    e = first_empty_from(s, i)
    e2 = first_empty_from(s, e + 1)
    s[e2], s[i] = s[i], (0, 0)                                                     # past an empty slot
    with pytest.raises(AssertionError, match="empty slot between"):
        check(good, slots=s, maxprobe=64)


def test_checker_refuses_maxprobe_one_too_small(good):
    with pytest.raises(AssertionError, match="maxprobe"):
        check(good, maxprobe=good["maxprobe"] - 1)


def test_checker_refuses_an_old_slot_moved(good):
    s = list(good["slots"])
    # two old members of one home slot change places: no hole, every distance within maxprobe, the same members
    assert s[9][1] and s[10][1] and s[9][0] & 63 == 9 == s[10][0] & 63 and s[9] in good["old_slots"] and s[10] in good["old_slots"]
    s[9], s[10] = s[10], s[9]
    with pytest.raises(AssertionError, match="old slot"):
        check(good, slots=s)


def test_checker_refuses_a_pool_prefix_byte_changed(good):
    p = list(good["pool"])
    p[len(good["old_pool"]) - 1] ^= 0x01
    with pytest.raises(AssertionError, match="prefix"):
        check(good, pool=p)


@pytest.mark.parametrize("off", [1, -1])
def test_checker_refuses_n_off_by_one(good, off):
    with pytest.raises(AssertionError, match="n = "):
        check(good, n=good["n"] + off)


def test_checker_refuses_a_ref_into_the_middle_of_an_entry(good):
    s = list(good["slots"])
    i = slot_of(good, good["last"])
    s[i] = (s[i][0], s[i][1] + 1)
    with pytest.raises(AssertionError, match="not the start"):
        check(good, slots=s)


def test_checker_refuses_a_table_that_is_too_small_or_no_power_of_two(good):
    with pytest.raises(AssertionError, match="power of two"):
        check(good, slots=good["slots"][:48], nslots=48)
    t = SM.Table([b"a", b"b"], SM.SEED)
    slots, pool, nslots, maxprobe, n, cnt = AM.set_add(t.slots, t.pool, t.n, t.maxprobe, SM.SEED, [b"c"])
    assert nslots == 8
    small = SM.Table([b"a", b"b", b"c"], SM.SEED)
    with pytest.raises(AssertionError, match="twice n"):
        AM.check_added(small.slots[:4], small.pool, 4, 3, 3, SM.SEED, t.slots, t.pool, [b"a", b"b", b"c"])


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("claim_set_add")
    AM.build_host(str(d / "claim_set_add_test"))
    AM.build_host(str(d / "claim_set_add_test_san"), sanitize=True)
    return d, str(d / "claim_set_add_test"), str(d / "claim_set_add_test_san")


def test_cpu_insertion_step_passes_the_checker_and_probes_as_python_in(exes):
    d, exe, san = exes
    cases = [(resident, SM.SEED, added, AM.queries_for(resident, added)) for _, resident, added in AM.directed_adds()]
    cases += [(resident, 0xffffffff, added, AM.queries_for(resident, added)) for _, resident, added in AM.directed_adds()[:6]]
    got = AM.run_host(exe, cases, d)
    for (resident, seed, added, queries), (before, after, hits) in zip(cases, got):
        t = SM.Table(resident, seed)
        assert (before["slots"], before["pool"], before["maxprobe"]) == (list(t.slots), t.pool, t.maxprobe)
        union = list(dict.fromkeys(resident + added))
        AM.check_added(after["slots"], after["pool"], after["nslots"], after["maxprobe"], after["n"], seed, t.slots, t.pool,
                       union, old_maxprobe=t.maxprobe)
        assert after["nslots"] == AM.grown_nslots(t.nslots, t.n, len(added))
        assert after["added"] == len(union) - t.n
        assert after["pool"] == AM.pack_delta(t.pool, added)[0]
        assert hits == [q in set(union) for q in queries], added[:3]
        if after["added"] == 0 and after["nslots"] == t.nslots:
            assert after["slots"] == list(t.slots) and len(after["pool"]) > len(t.pool)
    assert AM.run_host(san, cases, d, "san") == got


def test_cpu_refused_member_leaves_the_set(exes):
    d, exe, san = exes
    cases = [(resident, SM.SEED, members, resident + [m for m in members if SM.member_ok(m)])
             for _, resident, members, _ in AM.refused_adds()]
    for prog in (exe, san):
        got = AM.run_host(prog, cases, d, "refused")
        for (name, resident, members, k), (before, after, hits) in zip(AM.refused_adds(), got):
            assert after == ("rejected", k), name
            assert hits == [True] * len(resident) + [False] * (len(members) - 1), name
