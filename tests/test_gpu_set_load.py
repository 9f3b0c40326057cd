"""jg_set_load / jg_set_info / jg_set_free through the C ABI: load, info, free and
reload; a refused member and an injected allocation failure leave the set the
id named before answering; all sixteen ids.  Whether a set answers is asked the
way a caller asks: one jg_claims_match_set call on a payload that holds a
member.
"""
import pytest

from cap_amd import _lib
from tests import claims_corpus as CC
from tests import claims_match_set_cases as TC
from tests import set_model as SM
from tests.test_gpu_claims_scan import NOW

pytestmark = pytest.mark.gpu
IN = TC.IN_SET


@pytest.fixture()
def ctx():
    c = _lib.Context()
    yield c
    c.close()


def answers(ctx, set_id, values):
    """-> [is value a member of the loaded set] by one scan of payloads {"sid": value}"""
    segs = [CC.b64(b'{"sid":"' + v + b'","iat":%d,"exp":%d}' % (CC.T0, CC.T0 + 600)) for v in values]
    arena, jobs, o = b"", [], 0
    for s in segs:
        jobs.append((o, len(s), 0))
        arena += s
        o += len(s)
    codes, masks = ctx.claims_match_set(arena, jobs, [CC.resolve({}, NOW)], [[b"sid"]], [(0, IN, b"\0")], None, None, [set_id])
    assert set(codes) == {_lib.CL_OK}
    return [bool(m) for m in masks]


def test_load_info_free_reload(ctx):
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.set_info(3)
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.set_free(3)
    members = [b"a", b"bb", b"a", b"", b"ccc"]
    ctx.set_load(3, members, 99)
    t = SM.Table(members, 99)
    info = ctx.set_info(3)
    assert info == {"n": 4, "nslots": 8, "maxprobe": t.maxprobe, "seed": 99, "pool_bytes": 4 * len(t.pool), "generation": info["generation"]}
    assert answers(ctx, 3, [b"a", b"b", b"", b"ccc", b"cccc"]) == [True, False, True, True, False]
    ctx.set_load(3, [b"b"], 100)                                                 # loading an id in use replaces it
    assert ctx.set_info(3)["generation"] > info["generation"] and ctx.set_info(3)["n"] == 1 and ctx.set_info(3)["seed"] == 100
    assert answers(ctx, 3, [b"a", b"b", b""]) == [False, True, False]
    ctx.set_free(3)
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.set_info(3)
    with pytest.raises(_lib.JgError, match="not loaded"):
        answers(ctx, 3, [b"a"])
    ctx.set_load(3, [], 0)                                                       # the empty set is a set: it matches nothing
    assert ctx.set_info(3)["n"] == 0 and ctx.set_info(3)["nslots"] == 1 and ctx.set_info(3)["maxprobe"] == 0
    assert answers(ctx, 3, [b"a", b""]) == [False, False]
    for bad_id in (16, 17, 0xffffffff):
        with pytest.raises(_lib.JgError, match="rc=-1"):
            ctx.set_load(bad_id, [b"a"], 0)


@pytest.mark.parametrize("bad", [b"a\x80", b"\x1f", b'q"', b"back\\slash", b"x" * 256, b"\x7f"])
def test_refused_member_leaves_the_old_set_answering(ctx, bad):
    ctx.set_load(0, [b"old"], 1)
    before = ctx.set_info(0)
    with pytest.raises(_lib.JgError, match="rc=-1.*member 2"):
        ctx.set_load(0, [b"new", b"", bad, b"later"], 2)
    assert ctx.set_info(0) == before and answers(ctx, 0, [b"old", b"new"]) == [True, False]
    with pytest.raises(_lib.JgError, match="rc=-1.*member 1"):                   # a span past the bytes
        ctx.set_load(0, [b"new", b"x"], 2, spans=[(0, 3), (3, 2)])
    with pytest.raises(_lib.JgError, match="rc=-1"):                             # an id never loaded stays unloaded
        ctx.set_load(1, [bad], 2)
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.set_info(1)
    assert ctx.set_info(0) == before
    ctx.set_load(0, [b"x" * 255, b"new"], 2)                                     # the longest member is taken
    assert answers(ctx, 0, [b"old", b"new", b"x" * 255, b"x" * 254]) == [False, True, True, False]


@pytest.mark.parametrize("nth", [1, 2])
def test_injected_allocation_failure_leaves_the_old_set_answering(ctx, nth):
    ctx.set_load(5, [b"old", b"older"], 1)
    before = ctx.set_info(5)
    ctx.debug_fail_alloc(nth)                                                    # the table's allocation, or the pool's
    with pytest.raises(_lib.JgError, match="rc=-2.*out of memory"):
        ctx.set_load(5, [b"new"], 2)
    ctx.debug_fail_alloc(0)
    assert ctx.set_info(5) == before and answers(ctx, 5, [b"old", b"new", b"older"]) == [True, False, True]
    ctx.debug_fail_alloc(nth)
    with pytest.raises(_lib.JgError, match="rc=-2"):                             # ... and an id never loaded stays unloaded
        ctx.set_load(6, [b"new"], 2)
    ctx.debug_fail_alloc(0)
    with pytest.raises(_lib.JgError, match="rc=-1"):
        ctx.set_info(6)
    ctx.set_load(5, [b"new"], 2)                                                 # then a load goes through
    assert ctx.set_info(5)["generation"] == before["generation"] + 1
    assert answers(ctx, 5, [b"old", b"new"]) == [False, True]


def test_sixteen_ids(ctx):
    for i in range(16):
        ctx.set_load(i, [b"member-%d" % i, b"all"], i)
    gens = [ctx.set_info(i)["generation"] for i in range(16)]
    assert gens == sorted(gens) and len(set(gens)) == 16
    values = [b"member-%d" % i for i in range(16)] + [b"all", b"none"]
    for i in range(16):
        assert answers(ctx, i, values) == [k == i for k in range(16)] + [True, False], i
    # four of them in one call, by index
    seg = CC.b64(b'{"sid":"member-9","exp":%d}' % (CC.T0 + 600))
    codes, masks = ctx.claims_match_set(seg, [(0, len(seg), 0)], [CC.resolve({}, NOW)], [[b"sid"]],
                                        [(0, IN, bytes([x])) for x in range(4)], None, None, [15, 9, 0, 9])
    assert masks == [0b1010]
    for i in range(0, 16, 2):
        ctx.set_free(i)
    for i in range(16):
        if i % 2:
            assert ctx.set_info(i)["n"] == 2
        else:
            with pytest.raises(_lib.JgError, match="rc=-1"):
                ctx.set_info(i)
