"""Checker and sequential reference for members added to a resident set on the
device (cap_amd/csrc/kernels/claim_set_insert.hpp, jg_set_add).

The lanes of an insert launch race, so where inside its probe run a member lands
is free and there is no byte-for-byte model of the result as tests/set_model.py
is of a load.  check_added() states instead what every legal result has; set_add()
produces one legal result, sequentially.  Slots are (hash, ref) pairs and the
pool a list of dwords, as in set_model.py; the hash is set_model's.
"""
import functools
import os
import shutil
import struct
import subprocess

from tests import set_model as SM

ROOT = SM.ROOT


def pack_entry(m):
    m = bytes(m)
    padded = m + b"\0" * (-len(m) % 4)
    return [len(m)] + list(struct.unpack("<%dI" % (len(padded) // 4), padded))


def pack_delta(old_pool, members):
    """The pool with one entry per member of `members` packed behind old_pool, repeats included, and each one's ref
    -> (pool, refs): what the host hands the insert kernel"""
    pool, refs = list(old_pool), []
    for m in members:
        refs.append(len(pool) + 1)
        pool += pack_entry(m)
    return pool, refs


def entries(pool):
    """{dword index of an entry: its member} walking the pool end to end; raises on a malformed pool"""
    out, at = {}, 0
    while at < len(pool):
        ln = pool[at]
        assert ln <= SM.MEMBER_MAX, "entry at %d: length %d" % (at, ln)
        words = pool[at + 1:at + 1 + (ln + 3) // 4]
        assert len(words) == (ln + 3) // 4, "entry at %d runs past the pool" % at
        raw = struct.pack("<%dI" % len(words), *words)
        assert raw[ln:] == b"\0" * (len(raw) - ln), "entry at %d: padding not zero" % at
        out[at] = raw[:ln]
        at += 1 + len(words)
    return out


def grown_nslots(old_nslots, n_old, n_given):
    """The slot count jg_set_add chooses: the old one while it holds twice the members before plus those given"""
    if 2 * (n_old + n_given) <= old_nslots:
        return old_nslots
    ns = 1
    while ns < 2 * (n_old + n_given):
        ns *= 2
    return ns


def _longest_probe(slots, nslots):
    mask, longest = nslots - 1, 0
    for i, (h, ref) in enumerate(slots):
        if ref:
            longest = max(longest, ((i - (h & mask)) & mask) + 1)
    return longest


def check_added(slots, pool, nslots, maxprobe, n, seed, old_slots, old_pool, expected_members, old_maxprobe=None):
    """Raises AssertionError unless (slots, pool, nslots, maxprobe, n) is a legal result of adding to
    (old_slots, old_pool) under `seed` so that the set holds exactly expected_members.  old_maxprobe: the set's before;
    by default the longest probe run of old_slots, which is what a load or an add reports."""
    slots, pool, old_slots, old_pool = [tuple(s) for s in slots], list(pool), [tuple(s) for s in old_slots], list(old_pool)
    expected = [bytes(m) for m in expected_members]
    assert len(set(expected)) == len(expected), "expected_members repeats one"
    # 1
    assert nslots >= 1 and nslots & (nslots - 1) == 0, "nslots %d is no power of two" % nslots
    assert len(slots) == nslots, "%d slots given, nslots %d" % (len(slots), nslots)
    assert nslots >= 2 * n, "nslots %d under twice n = %d" % (nslots, n)
    # 2
    assert pool[:len(old_pool)] == old_pool and len(pool) >= len(old_pool), "the old pool is not a prefix of the new one"
    # 3
    ent = entries(pool)
    mask = nslots - 1
    named = []
    for i, (h, ref) in enumerate(slots):
        if not ref:
            assert h == 0, "slot %d: empty with hash %#x" % (i, h)
            continue
        assert ref - 1 in ent, "slot %d: ref %d is not the start of an entry" % (i, ref)
        m = ent[ref - 1]
        assert h == SM.set_hash(m, seed), "slot %d: hash %#x is not that of %r" % (i, h, m)
        named.append(m)
    # 4
    assert len(set(named)) == len(named), "a member has two slots: %r" % [m for m in set(named) if named.count(m) > 1][:3]
    assert set(named) == set(expected), ("members differ", sorted(set(expected) - set(named))[:3], sorted(set(named) - set(expected))[:3])
    assert n == len(named), "n = %d, %d slots occupied" % (n, len(named))
    # 5
    for i, (h, ref) in enumerate(slots):
        if not ref:
            continue
        dist = (i - (h & mask)) & mask
        assert dist + 1 <= maxprobe, "slot %d lies %d from home, maxprobe %d" % (i, dist, maxprobe)
        for k in range(dist):
            assert slots[((h & mask) + k) & mask][1], "slot %d: an empty slot between its home %d and itself" % (i, h & mask)
    if not named:
        assert maxprobe >= 0
    # 6, 7
    if len(old_slots) == nslots:
        for i, s in enumerate(old_slots):
            if s[1]:
                assert slots[i] == s, "old slot %d moved or changed" % i
        before = _longest_probe(old_slots, nslots) if old_maxprobe is None else old_maxprobe
        assert maxprobe >= before, "maxprobe %d below the old set's %d" % (maxprobe, before)
    else:
        assert nslots > len(old_slots), "the table shrank"
        now = set(slots)
        for i, s in enumerate(old_slots):
            if s[1]:
                assert s in now, "old slot %d is not in the new table" % i


def set_add(old_slots, old_pool, n_old, old_maxprobe, seed, members):
    """One legal result, members taken in order -> (slots, pool, nslots, maxprobe, n, added)"""
    members = [bytes(m) for m in members]
    assert all(SM.member_ok(m) for m in members)
    pool, refs = pack_delta(old_pool, members)
    ent = entries(pool)
    nslots = grown_nslots(len(old_slots), n_old, len(members))
    mask = nslots - 1
    if nslots == len(old_slots):
        slots, maxprobe = [tuple(s) for s in old_slots], old_maxprobe
    else:
        slots, maxprobe = [(0, 0)] * nslots, 0
        for h, ref in old_slots:
            if ref:
                i, probe = h & mask, 1
                while slots[i][1]:
                    i, probe = (i + 1) & mask, probe + 1
                slots[i] = (h, ref)
                maxprobe = max(maxprobe, probe)
    added = 0
    for m, ref in zip(members, refs):
        h = SM.set_hash(m, seed)
        i, probe = h & mask, 1
        while slots[i][1] and not (slots[i][0] == h and ent[slots[i][1] - 1] == m):
            i, probe = (i + 1) & mask, probe + 1
            assert probe <= nslots
        if not slots[i][1]:
            slots[i] = (h, ref)
            added += 1
            maxprobe = max(maxprobe, probe)
    return slots, pool, nslots, maxprobe, n_old + added, added


def contains(slots, pool, nslots, maxprobe, seed, q):
    """set_probe's walk over (slots, pool)"""
    q = bytes(q)
    h, mask = SM.set_hash(q, seed), nslots - 1
    i = h & mask
    for _ in range(maxprobe):
        sh, ref = slots[i]
        if not ref:
            return False
        if sh == h and pool[ref - 1] == len(q):
            words = pool[ref:ref + (len(q) + 3) // 4]
            if struct.pack("<%dI" % len(words), *words)[:len(q)] == q:
                return True
        i = (i + 1) & mask
    return False


@functools.lru_cache(maxsize=1)
def directed_adds():
    """[(name, resident members, members added in one call)] under SM.SEED: the adds the CPU program and the GPU tests
    share.  Every member is one the device accepts; the refused ones are refused_adds()."""
    pairs = SM.colliding_pairs()
    ids = lambda a, b: [b"id-%d" % k for k in range(a, b)]
    long_ = bytes(0x23 + (j * 7) % 0x5b for j in range(255)).replace(b"\\", b"/")
    home7 = SM._with_home(7, 8, 3)
    cases = [("to-the-empty-set", [], [b"a"]),
             ("empty-set-three", [], [b"a", b"b", b"c"]),
             ("one-member", ids(0, 5), [b"new"]),
             ("fill-to-half", ids(0, 5), ids(5, 8)),                       # 8 of 16 slots: no growth
             ("one-more-doubles", ids(0, 8), [b"id-8"]),                   # 9 members: 16 -> 32 slots
             ("three-doublings", ids(0, 8), ids(8, 64)),                   # 64 members: 16 -> 128 slots
             ("empty-string-and-255", [b"a"], [b"", long_]),
             ("255-resident-254-added", [long_], [long_[:254], long_[:254] + b"~", long_]),
             ("all-resident", ids(0, 5), [b"id-4", b"id-0", b"id-2"]),         # 8 given and resident: 16 slots hold them
             ("all-resident-grows", ids(0, 8), list(reversed(ids(0, 8)))),     # sized by what is given: rehashed, none added
             ("one-string-64-times", ids(0, 129), [b"again"] * 64),            # 512 slots: no growth
             ("one-string-64-times-grows", ids(0, 3), [b"again"] * 64),
             ("64-of-one-home-grows", ids(0, 64), SM._with_home(5, 256, 64, avoid=ids(0, 64))),
             ("28-of-one-home", ids(0, 100), SM._with_home(250, 256, 28, avoid=ids(0, 100))),
             ("same-state-pairs", [p[0] for p in pairs[:6]] + ids(0, 10), [p[1] for p in pairs[:6]]),
             ("same-state-pairs-grow", [p[0] for p in pairs[:6]], [p[1] for p in pairs[:6]] + [pairs[0][0]]),
             ("wraps", home7[:2] + [b"elsewhere"], home7[2:])]
    for name, resident, added in cases:
        assert all(SM.member_ok(m) for m in resident + added), name
    return cases


def refused_adds():
    """[(name, resident, members, index of the refused one)]"""
    return [("refused-first", [b"a", b"b"], [b"bad\x7f", b"c", b"d"], 0),
            ("refused-last", [b"a", b"b"], [b"c", b"d", b'q"'], 2)]


def queries_for(resident, added):
    qs = list(dict.fromkeys(list(resident) + list(added)))
    known = set(qs)
    non = [m + b"x" for m in qs] + [m[:-1] for m in qs if m] + [b"nope", b"", b"id-", b"x" * 255]
    non += [p[1] for p in SM.colliding_pairs()[:6]] + [p[0] for p in SM.colliding_pairs()[:6]]
    return qs + [q for q in dict.fromkeys(non) if q not in known]


def build_host(exe, sanitize=False):
    """Compile tests/host_unit/claim_set_add_test.cpp (the insertion and rehash steps for the CPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the insertion step's host program"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    src = os.path.join(ROOT, "tests", "host_unit", "claim_set_add_test.cpp")
    r = subprocess.run([cxx] + flags + ["-o", exe, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


def _words(hx):
    raw = b"" if hx == "-" else bytes.fromhex(hx)
    return list(struct.unpack("<%dI" % (len(raw) // 4), raw))


def parse_table(fields):
    """("T", n, nslots, maxprobe, slots hex, pool hex[, added]) -> dict"""
    assert fields[0] == "T", fields[:2]
    sw = _words(fields[4])
    d = dict(n=int(fields[1]), nslots=int(fields[2]), maxprobe=int(fields[3]),
             slots=[(sw[2 * k], sw[2 * k + 1]) for k in range(len(sw) // 2)], pool=_words(fields[5]))
    if len(fields) > 6:
        d["added"] = int(fields[6])
    return d


def run_host(exe, cases, workdir, name="adds"):
    """cases: [(resident, seed, added, queries)] -> [(table before, table after or ("rejected", k), [bool per query])]"""
    path = os.path.join(str(workdir), name + ".txt")
    with open(path, "w") as f:
        for resident, seed, added, queries in cases:
            f.write(" ".join(["B", "%d" % seed] + [SM._hex(m) for m in resident]) + "\n")
            f.write(" ".join(["A"] + [SM._hex(m) for m in added]) + "\n")
            for q in queries:
                f.write("Q %s\n" % SM._hex(q))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    lines = iter(r.stdout.splitlines())
    out = []
    for resident, seed, added, queries in cases:
        before = parse_table(next(lines).split())
        head = next(lines).split()
        after = parse_table(head) if head[0] == "T" else (head[0], int(head[1]))
        out.append((before, after, [next(lines) == "1" for _ in queries]))
    assert next(lines, None) is None
    return out
