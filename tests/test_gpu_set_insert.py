"""k_set_rehash and k_set_insert (kernels/claim_set_insert.hip) alone on the
device, through libcapjwt_tk.so's tk_set_insert and the production launchers:
every resulting table must pass tests/set_add_model.py's checker, and every
member and as many non-members are then asked through tk_set_probe and compared
with Python's `in`.

* The directed adds of tests/test_set_add_model.py: the empty set, one member,
  a fill to exactly half the slots, one and three doublings, "" and 255 bytes,
  members all resident, one string 64 times (one wave racing for one slot), 64
  strings of one home slot, same-state collision pairs split between resident
  and added, a chain that wraps.
* 65,536 members added to 65,536, with and without growth: many blocks and XCDs.
* 4,096 copies of each of 16 strings in one add.
* Input the kernels could leave their buffers on is refused before the launch.
"""
import array
import ctypes
import os

import pytest

from cap_amd import _lib
from tests import set_add_model as AM
from tests import set_model as SM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tk():
    L = ctypes.CDLL(os.path.join(ROOT, "cap_amd", "libcapjwt_tk.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.tk_set_probe.argtypes = [vp, u32, vp, u32, u32, u32, vp, ctypes.c_uint64, vp, ctypes.c_int64, vp]
    L.tk_set_insert.argtypes = [vp, u32, u32, vp, u32, vp, u32, u32, u32, vp, vp, vp]
    return L


def _u32(words, least=1):
    a = array.array("I", words)
    assert a.itemsize == 4
    buf = (ctypes.c_uint32 * max(least, len(a)))()
    if len(a):
        ctypes.memmove(buf, a.buffer_info()[0], 4 * len(a))
    return buf


def insert(tk, old_slots, old_pool, old_maxprobe, seed, members, new_nslots, pool=None, refs=None):
    """-> (rc, slots, pool, (added, maxprobe, error)); pool / refs override what pack_delta makes (for the argument checks)"""
    p, r = AM.pack_delta(old_pool, members)
    p, r = (p if pool is None else pool), (r if refs is None else refs)
    sout, pout, wout = _u32([0xeeeeeeee] * (2 * new_nslots)), _u32([0xeeeeeeee] * len(p)), _u32([0xeeeeeeee] * 3)
    rc = tk.tk_set_insert(_u32([w for s in old_slots for w in s]), len(old_slots), new_nslots, _u32(p), len(p), _u32(r), len(r),
                          old_maxprobe, seed, sout, pout, wout)
    sw = list(sout)
    return rc, [(sw[2 * k], sw[2 * k + 1]) for k in range(new_nslots)], list(pout)[:len(p)], tuple(wout)


def probe(tk, slots, pool, maxprobe, seed, queries):
    blob = b"".join(queries)
    sp = (_lib.JgSArg * len(queries))()
    o = 0
    for x, qy in zip(sp, queries):
        x.off, x.len = o, len(qy)
        o += len(qy)
    out = ctypes.create_string_buffer(b"\xee" * len(queries), len(queries))
    rc = tk.tk_set_probe(_u32([w for s in slots for w in s]), len(slots), _u32(pool), len(pool), maxprobe, seed, blob or b"\0",
                         len(blob), ctypes.cast(sp, ctypes.c_void_p), len(queries), out)
    assert rc == 0
    return list(out.raw)


def add_and_check(tk, old_slots, old_pool, n_old, old_maxprobe, seed, resident, added, name, non_members=None):
    new_nslots = AM.grown_nslots(len(old_slots), n_old, len(added))
    rc, slots, pool, (cnt, maxprobe, err) = insert(tk, old_slots, old_pool, old_maxprobe, seed, added, new_nslots)
    assert rc == 0 and err == 0, name
    union = list(dict.fromkeys(list(resident) + list(added)))
    assert cnt == len(union) - n_old, name
    assert pool == AM.pack_delta(old_pool, added)[0], name                       # the kernels write no pool byte
    AM.check_added(slots, pool, new_nslots, maxprobe, n_old + cnt, seed, old_slots, old_pool, union, old_maxprobe=old_maxprobe)
    qs = AM.queries_for(resident, added) if non_members is None else union + non_members
    known = set(union)
    want = [1 if qy in known else 0 for qy in qs]
    assert sum(want) == len(union) and want.count(0) >= min(len(union), 4), name
    hits = probe(tk, slots, pool, maxprobe, seed, qs)
    assert hits == want, (name, [(qy, h, w) for qy, h, w in zip(qs, hits, want) if h != w][:3])
    return slots, pool, maxprobe, cnt


def test_directed_adds_pass_the_checker_and_answer_as_python_in(tk):
    for name, resident, added in AM.directed_adds():
        t = SM.Table(resident, SM.SEED)
        slots, pool, maxprobe, cnt = add_and_check(tk, t.slots, t.pool, t.n, t.maxprobe, SM.SEED, resident, added, name)
        if cnt == 0 and len(slots) == t.nslots:
            assert slots == list(t.slots) and maxprobe == t.maxprobe and len(pool) > len(t.pool), name


@pytest.fixture(scope="module")
def big():
    name = lambda k, salt: b"jti-%08x-%d" % ((k * 2654435761 + salt) & 0xffffffff, k % 1000)
    resident = [name(k, 0) for k in range(65536)]
    added = [name(k, 0x9e3779b9) for k in range(65536)]
    non = [name(k, 0x3c6ef372) + b"!" for k in range(131072)]
    assert len(set(resident + added)) == 131072
    return resident, added, non


def test_65536_added_to_65536_with_growth(tk, big):
    resident, added, non = big
    t = SM.Table(resident, 0x1234abcd)
    assert t.nslots == 131072
    slots, pool, maxprobe, cnt = add_and_check(tk, t.slots, t.pool, t.n, t.maxprobe, 0x1234abcd, resident, added, "grow", non)
    assert cnt == 65536 and len(slots) == 262144


def test_65536_added_to_65536_without_growth(tk, big):
    resident, added, non = big
    # the residents in a table that already has room: made by the reference add into an empty table of 2^18 slots
    s0, p0, ns0, mp0, n0, _ = AM.set_add([(0, 0)] * 262144, [], 0, 0, 0x1234abcd, resident)
    assert (ns0, n0) == (262144, 65536)
    slots, pool, maxprobe, cnt = add_and_check(tk, s0, p0, n0, mp0, 0x1234abcd, resident, added, "no growth", non)
    assert cnt == 65536 and len(slots) == 262144 and maxprobe >= mp0


def test_4096_copies_of_16_strings(tk):
    resident = [b"id-%d" % k for k in range(100)]
    sixteen = [b"revoked-%d" % k for k in range(15)] + [b"id-7"]                  # one of them resident
    added = [sixteen[k % 16] for k in range(65536)]
    t = SM.Table(resident, SM.SEED)
    slots, pool, maxprobe, cnt = add_and_check(tk, t.slots, t.pool, t.n, t.maxprobe, SM.SEED, resident, added, "copies")
    assert cnt == 15 and len(slots) == 262144


def test_unsafe_input_is_refused_before_the_launch(tk):
    t = SM.Table([b"abc", b"defgh"], SM.SEED)
    untouched = (0xeeeeeeee,) * 3
    ok = insert(tk, t.slots, t.pool, t.maxprobe, SM.SEED, [b"x"], 8)
    assert ok[0] == 0 and ok[3][0] == 1 and ok[3][2] == 0
    p, r = AM.pack_delta(t.pool, [b"wxyz"])
    bad = lambda **kw: insert(tk, kw.pop("slots", t.slots), t.pool, kw.pop("maxprobe", t.maxprobe), SM.SEED, [b"wxyz"],
                              kw.pop("nslots", 8), **kw)
    for got in (bad(nslots=2),                                                   # a table that shrinks
                bad(nslots=12),                                                  # no power of two
                bad(nslots=4),                                                   # three members in four slots
                bad(slots=t.slots[:3]),
                bad(maxprobe=5),
                bad(refs=[r[0] + 1]),                                            # a ref into the middle of an entry
                bad(refs=[0]),
                bad(refs=[len(p) + 1]),                                          # past the pool
                bad(pool=p[:-1]),                                                # the last entry runs past the pool
                bad(pool=[256] + p[1:]),                                         # a length over JG_SET_MEMBER_MAX
                bad(slots=[(h, ref + 1 if ref else 0) for h, ref in t.slots])):  # a resident ref into an entry
        assert got[0] == -1 and got[3] == untouched
