"""The resident set's host code (kernels/claim_set.hpp: set_build, set_probe, the
hash) against its plain-Python model (tests/set_model.py), without a GPU:

- the table set_build() makes is the model's, byte for byte, for every directed
  build: sizes around every doubling of the slot count, "", duplicates, 255-byte
  members, two members of one 32-bit hash, members that share a home slot, a
  chain that wraps past the last slot, a non-member with a member's hash;
- set_probe() and the model's probe agree with Python's `in` for every member
  and for the strings around them;
- the directed builds have the properties they are named for;
- members the device refuses are refused, naming the member;
- the stand-alone program built with ASan + UBSan prints the same.
"""
import random

import pytest

from tests import set_model as SM


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("claim_set")
    SM.build_host(str(d / "claim_set_test"))
    SM.build_host(str(d / "claim_set_test_san"), sanitize=True)
    return d, str(d / "claim_set_test"), str(d / "claim_set_test_san")


def test_colliding_pairs_exist_and_collide():
    pairs = SM.colliding_pairs()
    assert len(pairs) >= 6                                               # about 18 are expected
    for a, b in pairs:
        assert a != b and SM.set_hash(a, SM.SEED) == SM.set_hash(b, SM.SEED)
    # the seed is folded in where the hash is finalised: it moves the pair, together
    assert SM.set_hash(pairs[0][0], SM.SEED + 1) == SM.set_hash(pairs[0][1], SM.SEED + 1) != SM.set_hash(pairs[0][0], SM.SEED)
    assert SM.hash_state(b"") == SM.BASIS and SM.set_hash(b"", 0) != SM.set_hash(b"", 1)


def test_model_probe_is_python_in():
    for name, members, queries in SM.directed_builds():
        t = SM.Table(members, SM.SEED)
        s = set(members)
        assert t.n == len(s) and t.nslots >= max(1, 2 * t.n) and t.nslots & (t.nslots - 1) == 0, name
        assert t.nslots == 1 or t.nslots < 4 * t.n, name
        assert sum(1 for _, ref in t.slots if ref) == t.n, name
        for q in queries:
            assert (q in t) == (q in s), (name, q)
        assert all(m in t for m in members), name


def test_directed_builds_are_what_they_are_named_for():
    B = {name: (SM.Table(members, SM.SEED), members, queries) for name, members, queries in SM.directed_builds()}
    assert [B["size-%d" % n][0].nslots for n in (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)] == \
        [1, 2, 4, 8, 8, 16, 16, 32, 32, 64, 64, 128, 128, 256]
    assert B["size-0"][0].maxprobe == 0 and B["size-0"][0].pool == [] and b"" not in B["size-0"][0]
    assert b"" in B["empty-string"][0] and b"" in B["only-empty-string"][0] and B["only-empty-string"][0].pool == [0]
    assert B["duplicates"][0].n == 4
    assert all(len(m) == 255 for m in B["255-bytes"][1][:4]) and B["255-bytes"][0].n == 5
    t, members, _ = B["same-hash"]
    assert SM.set_hash(members[0], SM.SEED) == SM.set_hash(members[2], SM.SEED) and t.maxprobe >= 2
    assert len({h for h, ref in t.slots if ref}) == 3                                        # five members, three hashes
    t, members, queries = B["hash-of-a-member"]
    for a, b in SM.colliding_pairs()[:6]:
        hit, compared = t.probe(b)
        assert a in t and not hit and b in queries and SM.set_hash(a, SM.SEED) == SM.set_hash(b, SM.SEED)
        assert compared == 1                                                                 # the hash and the length agreed: the bytes decided
    t, members, _ = B["shared-home"]
    assert t.maxprobe == 3 and [t.home[m] for m in members[:3]] == [(2, 2), (2, 3), (2, 4)]
    t, members, _ = B["wraps"]
    assert [t.home[m][1] for m in members] == [7, 0, 1, 2] and t.maxprobe == 3 and t.home[members[3]][0] == 0


def test_host_build_is_the_model_byte_for_byte(exes):
    d, exe, san = exes
    builds = [(members, SM.SEED, queries) for _, members, queries in SM.directed_builds()]
    rnd = random.Random(7)
    alphabet = bytes(c for c in range(0x20, 0x7f) if c not in (0x22, 0x5c))
    for n, seed in ((100, 0), (1000, 0xffffffff), (5000, 12345)):
        members = [bytes(rnd.choice(alphabet) for _ in range(rnd.randrange(0, 40))) for _ in range(n)]
        builds.append((members, seed, members[:50] + [m + b"!" for m in members[:50]]))
    got = SM.run_host(exe, builds, d)
    for (members, seed, queries), (head, hits) in zip(builds, got):
        t = SM.Table(members, seed)
        slots, pool = t.to_hex()
        assert head == ("T", str(t.n), str(t.nslots), str(t.maxprobe), slots, pool), members[:4]
        assert hits == [q in set(members) for q in queries]
    assert SM.run_host(san, builds, d, "san") == got


@pytest.mark.parametrize("bad", [b"a\x80", b"\x1f", b'q"', b"back\\slash", b"x" * 256, b"\x7f", b"nul\0"])
def test_refused_members_are_named(exes, bad):
    d, exe, san = exes
    assert not SM.member_ok(bad)
    for prog in (exe, san):
        (head, hits), = SM.run_host(prog, [([b"ok", b"", bad, b"later"], 1, [b"ok"])], d, "refused")
        assert head == ("rejected", "2") and hits == [False]
    assert SM.member_ok(b"x" * 255) and SM.member_ok(b" ~!#[]") and SM.member_ok(b"")
