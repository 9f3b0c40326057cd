"""The checker of tests/test_gpu_ec_xyzz_exact.py on the CPU: the device's
formulas in integers (xyzz_model.xyzz_chain) pass check_lane on every lane of
the GPU test, and an injected wrong sign fails it -- in the reference's inputs
(one step's sign flipped) and in the formulas (r = S2 + Y)."""
import pytest

from tests import xyzz_model as X


@pytest.fixture(scope="module")
def lanes():
    return X.build_lanes()


def test_lane_shapes(lanes):
    counts = {len(ln.points) for ln in lanes if not ln.exceptional}
    assert {1, 2, 3, 20} <= counts
    assert sum(ln.exceptional for ln in lanes) == 6
    first3 = {tuple(ln.signs[:3]) for ln in lanes if len(ln.points) >= 3 and 0 not in ln.signs[:3]}
    assert len(first3) == 8
    pts, sg, cnt = X.pack(lanes)
    assert len(pts) == len(lanes) * X.STEPS * 2 * X.L and len(sg) == len(lanes) * X.STEPS and len(cnt) == len(lanes)
    assert all(0 <= v < (1 << X.W) for v in pts)


def test_correct_chain_passes(lanes):
    for ln in lanes:
        X.check_lane(ln, *X.xyzz_chain(ln.points, ln.signs))


def test_wrong_sign_in_the_reference_fails(lanes):
    """every lane of two or more steps, each step's sign flipped in turn"""
    n = 0
    for ln in lanes:
        if ln.exceptional or len([s for s in ln.signs if s]) < 2:
            continue
        out = X.xyzz_chain(ln.points, ln.signs)
        for i, s in enumerate(ln.signs):
            if s == 0 or ln.points[i][1] == 0:        # y == 0 (a limb-extreme lane): -P is P
                continue
            flipped = list(ln.signs)
            flipped[i] = -s
            wrong = X.Lane(ln.tag, ln.points, flipped)
            with pytest.raises(AssertionError):
                X.check_lane(wrong, *out)
            n += 1
    assert n > 100


def test_wrong_sign_in_the_formulas_fails(lanes):
    n = 0
    for ln in lanes:
        if ln.exceptional or len([s for s in ln.signs if s]) < 2:
            continue
        with pytest.raises(AssertionError):
            X.check_lane(ln, *X.xyzz_chain(ln.points, ln.signs, r_sign=1))
        n += 1
    assert n > 30


def test_exceptional_lane_with_a_live_zz_fails(lanes):
    ln = next(x for x in lanes if x.exceptional)
    with pytest.raises(AssertionError):
        X.check_lane(ln, 5, 7, 1, 1, False)
