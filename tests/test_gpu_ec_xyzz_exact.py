"""The P-256 addition chain of k_ec_point on the XYZZ accumulator against
Python integers (GPU).

tk_ec_xyzz_chain (cap_amd/csrc/tests/tk_ec_xyzz.hip) runs add_ent with the
template arguments ec_point_token uses -- the assignment, madd_xyzz_z1 for the
second entry, madd_xyzz from the third -- on caller-supplied affine points
(canonical Montgomery limbs) with a sign per step and a count per lane, and
hands back X, Y, ZZ, ZZZ.  tests/xyzz_model.py builds one wave of lanes
(chains of 1, 2, 3 and 20 additions; random multiples of G; every sign pattern
of the first three steps; a skipped step; coordinates at the limb extremes;
steps that add P to P and to -P in the Z = 1 and the general form, each
followed by five further additions) and checks each lane: X / ZZ and Y / ZZZ
equal the chord-rule sum (for multiples of G also the scalar multiple),
ZZ^3 == ZZZ^2, and an exceptional step leaves ZZ == ZZZ == 0 for good.  The
reference is integer arithmetic, never another kernel; every comparison is
equality mod p.  The kernel runs once for the module.

Limb bounds asserted on the way out are the ones the next addition and the
accept test assume (ecdsa_impl.hpp madd_xyzz): 28-bit limbs everywhere, Y, ZZ,
ZZZ < 2p, X < 10p."""
import ctypes
import os

import numpy as np
import pytest

from tests import xyzz_model as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tk():
    lib = ctypes.CDLL(os.path.join(ROOT, "cap_amd", "libcapjwt_tk.so"))
    vp = ctypes.c_void_p
    lib.tk_ec_xyzz_chain.argtypes = [ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int]
    lib.tk_ec_xyzz_chain.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def run(tk):
    lanes = X.build_lanes()
    pts, sg, cnt = X.pack(lanes)
    pts, sg, cnt = np.array(pts, np.uint32), np.array(sg, np.int32), np.array(cnt, np.int32)
    out = np.full(len(lanes) * X.OUT_WORDS, 0xA5A5A5A5, np.uint32)
    rc = tk.tk_ec_xyzz_chain(1, pts.ctypes.data, sg.ctypes.data, cnt.ctypes.data, out.ctypes.data, len(lanes), X.STEPS)
    assert rc == 0
    return lanes, out.reshape(len(lanes), X.OUT_WORDS)


def coords(row):
    """(X, Y, ZZ, ZZZ) Montgomery values of a lane's output row, and its empty flag"""
    return [X.value(row[k * X.L:(k + 1) * X.L]) for k in range(4)], int(row[4 * X.L])


def lanes_where(run, pred):
    lanes, out = run
    sel = [(ln, out[i]) for i, ln in enumerate(lanes) if pred(ln)]
    assert sel
    return sel


def check(sel):
    for ln, row in sel:
        vals, empty = coords(row)
        assert empty in (0, 1), ln.tag
        X.check_lane(ln, *[X.from_mont(v % X.P) for v in vals], bool(empty))
        if not empty:
            assert all(int(w) < (1 << X.W) for w in row[:4 * X.L]), (ln.tag, "a limb over 28 bits")
            assert vals[0] < 10 * X.P and all(v < 2 * X.P for v in vals[1:]), (ln.tag, "value bound")


@pytest.mark.parametrize("n", [1, 2, 3, 20])
def test_chain_of_n_additions(run, n):
    check(lanes_where(run, lambda ln: not ln.exceptional and len(ln.points) == n))


def test_every_sign_pattern_of_the_first_three_steps(run):
    sel = lanes_where(run, lambda ln: ln.tag.startswith("signs "))
    assert {tuple(ln.signs[:3]) for ln, _ in sel} == {(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)}
    assert {len(ln.points) for ln, _ in sel} == {3, 20}
    check(sel)


def test_skipped_steps(run):
    check(lanes_where(run, lambda ln: 0 in ln.signs))


def test_coordinates_at_the_limb_extremes(run):
    sel = lanes_where(run, lambda ln: ln.tag.startswith("extreme"))
    assert len(sel) >= 11
    check(sel)


def test_exceptional_steps_leave_zz_zero_for_good(run):
    sel = lanes_where(run, lambda ln: ln.exceptional)
    assert sorted(len(ln.points) for ln, _ in sel) == [7, 7, 8, 8, 26, 26]
    check(sel)


def test_every_lane(run):
    check(lanes_where(run, lambda ln: True))


def test_hook_refuses_a_jacobian_curve(tk):
    """P-384 and P-521 keep the Jacobian accumulator: the hook has no chain for them"""
    z = np.zeros(4, np.uint32)
    for curve in (2, 3, 9):
        assert tk.tk_ec_xyzz_chain(curve, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1, 1) == -1
