"""Plain-Python model of a resident set (cap_amd/csrc/kernels/claim_set.hpp;
DESIGN.md 10.9): the hash (one running state for every set, seeded where it is
finalised), the table set_build() makes from (members, seed), and
set_probe()'s lookup.  Shared by the tests of the set itself and of the scan
that asks it.

Layout.  A slot is (hash, ref): the member's finalised 32-bit hash and the dword
index of its pool entry plus one; ref 0 is empty.  The slot count is the smallest
power of two that is at least twice the number of distinct members (1 for none).
Members are taken in the order given, a repeated one folded into its first
occurrence; each goes to the first empty slot from hash & mask on, upwards with
wrap-around.  A pool entry is the length as one dword and then the bytes,
little-endian, padded with zeros to a dword.  maxprobe is the longest run of
slots an insertion looked at, its own included.
"""
import functools
import os
import shutil
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xffffffff
MEMBER_MAX = 255                                                         # JG_SET_MEMBER_MAX
SEED = 0x5eed1234                                                        # the tests' fixed seed


def hash_step(h, c):
    return ((h ^ c) * 16777619) & M32


BASIS = 2166136261                                                       # kHashBasis: the state of the empty string


def hash_final(h, seed):
    h ^= seed & M32
    h ^= h >> 16
    h = (h * 0x85ebca6b) & M32
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & M32
    return h ^ (h >> 16)


def hash_state(b):
    h = BASIS
    for c in bytes(b):
        h = hash_step(h, c)
    return h


def set_hash(b, seed):
    return hash_final(hash_state(b), seed)


def member_ok(m):
    return len(m) <= MEMBER_MAX and all(0x20 <= c <= 0x7e and c not in (0x22, 0x5c) for c in bytes(m))


class Table:
    def __init__(self, members, seed):
        distinct = list(dict.fromkeys(bytes(m) for m in members))
        assert all(member_ok(m) for m in distinct)
        self.seed, self.n = seed & M32, len(distinct)
        self.nslots = 1
        while self.nslots < 2 * self.n:
            self.nslots *= 2
        self.slots = [(0, 0)] * self.nslots
        self.pool, self.maxprobe = [], 0
        self.home = {}                                                   # member -> (home slot, slot it lies at)
        mask = self.nslots - 1
        for m in distinct:
            h = set_hash(m, self.seed)
            at = len(self.pool)
            self.pool.append(len(m))
            padded = m + b"\0" * (-len(m) % 4)
            self.pool += list(struct.unpack("<%dI" % (len(padded) // 4), padded))
            i, probe = h & mask, 1
            while self.slots[i][1]:
                i, probe = (i + 1) & mask, probe + 1
            self.slots[i] = (h, at + 1)
            self.home[m] = (h & mask, i)
            self.maxprobe = max(self.maxprobe, probe)

    def probe(self, q):
        """set_probe's walk -> (is a member, slots whose hash and length agreed and were compared)"""
        q = bytes(q)
        h, mask = set_hash(q, self.seed), self.nslots - 1
        i, compared = h & mask, 0
        for _ in range(self.maxprobe):
            sh, ref = self.slots[i]
            if not ref:
                return False, compared
            if sh == h and self.pool[ref - 1] == len(q):
                compared += 1
                words = self.pool[ref:ref + (len(q) + 3) // 4]
                if struct.pack("<%dI" % len(words), *words)[:len(q)] == q:
                    return True, compared
            i = (i + 1) & mask
        return False, compared

    def __contains__(self, q):
        return self.probe(q)[0]

    def slot_words(self):
        return [w for s in self.slots for w in s]

    def to_hex(self):
        """(slots, pool) as the host program prints them: little-endian bytes in hex, "-" for none"""
        f = lambda ws: struct.pack("<%dI" % len(ws), *ws).hex() if ws else "-"
        return f(self.slot_words()), f(self.pool)


@functools.lru_cache(maxsize=4)
def colliding_pairs(seed=SEED, count=400000):
    """Pairs of distinct eight-letter strings with the same 32-bit hash state, and so the same hash under `seed` and
    under every other: a birthday search over `count` strings (about count^2 / 2^33 pairs are expected: 18 for 4 * 10^5), with numpy, checked against the model.  The
    strings are scattered over all eight letters: among strings that differ in their last few bytes only, the
    xor-multiply has no collisions at all."""
    import numpy as np
    L, space = 8, 26 ** 8
    idx = (np.arange(count, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(space)
    h = np.full(count, BASIS, dtype=np.uint64)
    for d in range(L):
        c = (idx // np.uint64(26 ** (L - 1 - d))) % np.uint64(26) + np.uint64(97)
        h = ((h ^ c) * np.uint64(16777619)) & np.uint64(M32)
    order = np.argsort(h, kind="stable")
    hs = h[order]
    same = np.nonzero(hs[1:] == hs[:-1])[0]
    name = lambda k: bytes(97 + (int(k) // 26 ** (L - 1 - d)) % 26 for d in range(L))
    pairs = [(name(idx[order[j]]), name(idx[order[j + 1]])) for j in same]
    for a, b in pairs:
        assert a != b and set_hash(a, seed) == set_hash(b, seed)
    return pairs


def build_host(exe, sanitize=False):
    """Compile tests/host_unit/claim_set_test.cpp (set_build and set_probe for the CPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the set's host model"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    src = os.path.join(ROOT, "tests", "host_unit", "claim_set_test.cpp")
    r = subprocess.run([cxx] + flags + ["-o", exe, src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


_hex = lambda b: bytes(b).hex() or "-"


def run_host(exe, builds, workdir, name="sets"):
    """builds: [(members, seed, queries)] -> [(table line fields or ("rejected", k), [bool per query])]"""
    path = os.path.join(str(workdir), name + ".txt")
    with open(path, "w") as f:
        for members, seed, queries in builds:
            f.write(" ".join(["B", "%d" % seed] + [_hex(m) for m in members]) + "\n")
            for q in queries:
                f.write("Q %s\n" % _hex(q))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    lines = iter(r.stdout.splitlines())
    out = []
    for members, seed, queries in builds:
        head = next(lines).split()
        out.append((tuple(head), [next(lines) == "1" for _ in queries]))
    assert next(lines, None) is None
    return out


def _with_home(home, nslots, count, seed=SEED, avoid=()):
    """`count` short strings whose home slot in a table of `nslots` is `home`"""
    out, k = [], 0
    while len(out) < count:
        m = b"m%d" % k
        if set_hash(m, seed) & (nslots - 1) == home and m not in avoid:
            out.append(m)
        k += 1
    return out


@functools.lru_cache(maxsize=1)
def directed_builds():
    """[(name, members, queries)] under SEED: the builds the set's tests share.  Every build's queries hold all its
    members, and for each member the strings around it: a byte longer, a byte shorter, its last byte changed."""
    pairs = colliding_pairs()
    long_ = [bytes(0x23 + (i * 7 + j) % 0x5b for j in range(255)) for i in range(3)]
    long_ = [m.replace(b"\\", b"/") for m in long_]
    builds = [("size-%d" % n, [b"id-%d" % k for k in range(n)]) for n in (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)]
    builds += [("empty-string", [b"", b"a", b"ab"]),
               ("only-empty-string", [b""]),
               ("duplicates", [b"x", b"y", b"x", b"", b"z", b"y", b"", b"x"]),
               ("255-bytes", long_ + [long_[0][:254] + b"~", long_[1][:254]]),
               ("same-hash", [pairs[0][0], b"other", pairs[0][1], pairs[1][1], pairs[1][0]]),
               ("hash-of-a-member", [p[0] for p in pairs[:6]] + [b"plain"]),
               ("shared-home", _with_home(2, 8, 3) + [b"elsewhere"]),
               ("wraps", _with_home(7, 8, 3) + _with_home(0, 8, 1))]
    out = []
    for name, members in builds:
        qs = list(members)
        for m in dict.fromkeys(members):
            qs += [m + b"x", m[:-1], m[:-1] + bytes([m[-1] ^ 1]) if m else b" ", m[:len(m) // 2]]
        qs += [b"", b"nope", b"id-", b"\xc3\xa9", b"a\x80", b"x" * 255, b"x" * 256, b"x" * 300, long_[0] + b"!"]
        qs += [p[1] for p in pairs[:6]]
        out.append((name, members, qs))
    return out
