"""Which point kernel a launch of n padded tokens runs (kernels/point_form.hpp,
used by launch_chain and launch_ed), read through the test library as
(lanes per token, prefetching chain, persistent k_ec_point):
  (4, 0, 0)  k_ec_point_split<CV, 4, false> / k_ed_point_split<WA, 4>
  (2, 1, 0)  k_ec_point_split<CV, 2, true> (P-256)
  (1, 1, 0)  k_ec_point_split<CV, 1, true> / k_ed_point_pf
  (1, 0, 1)  k_ec_point, persistent with a capped grid (P-256)
  (1, 0, 0)  k_ec_point, one block per 64 tokens / k_ed_point
This pins the form at both sides of every size threshold, and the forms the
tiled launches of test_gpu_comb_tiers.py select (host code only, but it lives
in the device test library)."""
import ctypes
import os

import pytest

from tests import test_gpu_comb_tiers as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P256, P384, P521, ED = 4, 5, 6, 7          # kernels/common.hpp Cls
CLS = {"P-256": P256, "P-384": P384, "P-521": P521}

SPLIT4, SPLIT2_PF, ONE_PF, POINT, PERSISTENT = (4, 0, 0), (2, 1, 0), (1, 1, 0), (1, 0, 0), (1, 0, 1)
#     n:      P-256       P-384   P-521   Ed25519
TABLE = {
    64:      (SPLIT4,     SPLIT4, SPLIT4, SPLIT4),
    16384:   (SPLIT4,     SPLIT4, SPLIT4, SPLIT4),
    16448:   (SPLIT2_PF,  ONE_PF, ONE_PF, ONE_PF),
    65536:   (SPLIT2_PF,  ONE_PF, ONE_PF, ONE_PF),
    65600:   (SPLIT2_PF,  ONE_PF, POINT,  ONE_PF),
    131072:  (SPLIT2_PF,  ONE_PF, POINT,  ONE_PF),
    131136:  (ONE_PF,     ONE_PF, POINT,  POINT),
    262144:  (ONE_PF,     ONE_PF, POINT,  POINT),
    262208:  (PERSISTENT, POINT,  POINT,  POINT),
    1048576: (PERSISTENT, POINT,  POINT,  POINT),
}


@pytest.fixture(scope="module")
def tk():
    return ctypes.CDLL(os.path.join(ROOT, "cap_amd", "libcapjwt_tk.so"))


def _form(tk, cls, n, force=0):
    lanes, pf, pers = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = tk.tk_point_form(cls, ctypes.c_int64(n), force, ctypes.byref(lanes), ctypes.byref(pf), ctypes.byref(pers))
    assert rc == 0, (cls, n, force)
    return lanes.value, pf.value, pers.value


def test_point_form_table(tk):
    for n, want in TABLE.items():
        for cls, w in zip((P256, P384, P521, ED), want):
            assert _form(tk, cls, n) == w, (cls, n)
    # the debugging switch: k_ec_point at every size
    for n in (64, 1048576):
        assert _form(tk, P256, n, force=1) == PERSISTENT
        assert _form(tk, P384, n, force=1) == POINT
        assert _form(tk, P521, n, force=1) == POINT
    out = ctypes.c_int()
    o = ctypes.byref(out)
    for cls, n in ((3, 64), (8, 64), (P256, 0), (P256, -64), (P256, 100), (ED, 0), (ED, 100)):
        assert tk.tk_point_form(cls, ctypes.c_int64(n), 0, o, o, o) == -1, (cls, n)
    assert tk.tk_point_form(P256, ctypes.c_int64(64), 0, None, o, o) == -1


def test_comb_tier_launches_select_the_forms_their_docstrings_name(tk):
    fx = T.fixtures()
    mid, large = T.MID_LAUNCH_JOBS
    # test_ecdsa_comb_tier_mid_launch
    want = {("P-256", mid): SPLIT2_PF, ("P-256", large): ONE_PF,
            ("P-384", mid): ONE_PF, ("P-384", large): ONE_PF,
            ("P-521", mid): ONE_PF, ("P-521", large): POINT}
    seen = set()
    for s in fx["ec"]:
        for n in T.MID_LAUNCH_JOBS:
            padded = T._padded(T._tiled(s["tokens"], n))
            assert _form(tk, CLS[s["crv"]], padded) == want[(s["crv"], n)], (s["crv"], s["wq"], n, padded)
            seen.add((s["crv"], n))
    assert seen == set(want)
    # test_ed25519_comb_tier_large_launch
    small, large = T.ED_LARGE_LAUNCH_JOBS
    toks = fx["ed25519"]["tokens"]
    assert _form(tk, ED, T._padded(T._tiled(toks, small))) == ONE_PF
    assert _form(tk, ED, T._padded(T._tiled(toks, large))) == POINT
    # the plain tier tests run the 4-lane split
    assert _form(tk, ED, T._padded(toks)) == SPLIT4
    for s in fx["ec"]:
        assert _form(tk, CLS[s["crv"]], T._padded(s["tokens"])) == SPLIT4
