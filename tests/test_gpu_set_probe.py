"""set_probe (kernels/claim_set.hpp) alone on the device, through
libcapjwt_tk.so's tk_set_probe: one lane per query string against a table made
by tests/set_model.py, every answer against Python's `in`.

* The directed builds of tests/test_set_model.py: sizes around every doubling of
  the slot count, "", duplicates, 255-byte members, two members of one 32-bit
  hash, a shared home slot, a chain that wraps, a non-member with a member's hash.
* One set of 65,536 members with 4,096 queries, half of them members.
* jg_set_load's table and pool, read back from the device, are the model's,
  byte for byte.
* A table or queries that could lead a lookup out of its buffers are refused
  before the launch.
"""
import ctypes
import os

import pytest

from cap_amd import _lib
from tests import set_model as SM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tk():
    L = ctypes.CDLL(os.path.join(ROOT, "cap_amd", "libcapjwt_tk.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.tk_set_probe.argtypes = [vp, u32, vp, u32, u32, u32, vp, ctypes.c_uint64, vp, ctypes.c_int64, vp]
    return L


def probe(tk, t, queries, slots=None, pool=None, maxprobe=None, spans=None):
    """-> (rc, [hit per query]); slots / pool / maxprobe / spans override the model's (for the argument checks)"""
    sw = t.slot_words() if slots is None else slots
    pw = t.pool if pool is None else pool
    blob = b"".join(queries)
    if spans is None:
        spans, o = [], 0
        for qy in queries:
            spans.append((o, len(qy)))
            o += len(qy)
    sp = (_lib.JgSArg * max(1, len(spans)))()
    for x, (off, ln) in zip(sp, spans):
        x.off, x.len = off, ln
    out = ctypes.create_string_buffer(b"\xee" * len(spans), len(spans))
    rc = tk.tk_set_probe((ctypes.c_uint32 * len(sw))(*sw), len(sw) // 2, (ctypes.c_uint32 * max(1, len(pw)))(*pw), len(pw),
                         t.maxprobe if maxprobe is None else maxprobe, t.seed, blob or b"\0", len(blob),
                         ctypes.cast(sp, ctypes.c_void_p), len(spans), out)
    return rc, list(out.raw)


def test_directed_builds_answer_as_python_in(tk):
    for name, members, queries in SM.directed_builds():
        t = SM.Table(members, SM.SEED)
        rc, hits = probe(tk, t, queries)
        assert rc == 0, name
        want = [1 if qy in set(members) else 0 for qy in queries]
        assert hits == want, (name, [(qy, h, w) for qy, h, w in zip(queries, hits, want) if h != w][:3])
        assert sum(want) >= len(set(members)) and (0 in want)


def test_65536_members_4096_queries(tk):
    members = [b"jti-%08x-%d" % ((k * 2654435761) & 0xffffffff, k % 1000) for k in range(65536)]
    t = SM.Table(members, 0x1234abcd)
    assert t.n == 65536 and t.nslots == 131072 and t.maxprobe >= 3
    queries = [members[(k * 31) % 65536] if k % 2 == 0 else b"jti-%08x-%d" % ((k * 40503) & 0xffffffff, 1000 + k) for k in range(4096)]
    s = set(members)
    want = [1 if qy in s else 0 for qy in queries]
    assert sum(want) == 2048
    rc, hits = probe(tk, t, queries)
    assert rc == 0 and hits == want


def test_loaded_table_is_the_model_byte_for_byte():
    ctx = _lib.Context()
    try:
        for k, (name, members, _) in enumerate(SM.directed_builds()):
            ctx.set_load(k % 16, members, SM.SEED)
            t = SM.Table(members, SM.SEED)
            slots, pool = ctx.set_read(k % 16)
            assert [w for s in slots for w in s] == t.slot_words() and pool == t.pool, name
            info = ctx.set_info(k % 16)
            assert (info["n"], info["nslots"], info["maxprobe"], info["seed"], info["pool_bytes"]) == \
                (t.n, t.nslots, t.maxprobe, SM.SEED, 4 * len(t.pool)), name
    finally:
        ctx.close()


def test_unsafe_tables_and_queries_are_refused(tk):
    t = SM.Table([b"abc", b"defgh"], SM.SEED)
    sw, pw = t.slot_words(), t.pool
    untouched = (-1, [0xee])
    assert probe(tk, t, [b"abc"]) == (0, [1])
    assert probe(tk, t, [b"abc"], slots=sw[:6]) == untouched                      # three slots: no power of two
    assert probe(tk, t, [b"abc"], maxprobe=5) == untouched                         # more probes than slots
    used = [k for k in range(t.nslots) if sw[2 * k + 1]]
    bad = list(sw)
    bad[2 * used[0] + 1] = len(pw) + 1                                             # a ref past the pool
    assert probe(tk, t, [b"abc"], slots=bad) == untouched
    assert probe(tk, t, [b"abc"], pool=pw[:-1]) == untouched                       # an entry that runs past it
    assert probe(tk, t, [b"abc"], pool=[256] + pw[1:]) == untouched                # a length over JG_SET_MEMBER_MAX
    assert probe(tk, t, [b"abc"], spans=[(1, 3)]) == untouched                     # a query past the query bytes
    assert probe(tk, t, [b"abc"], spans=[(4, 0)]) == untouched
    assert probe(tk, t, [b"abc"], spans=[(3, 0)]) == (0, [0])                      # "" at the very end is inside
