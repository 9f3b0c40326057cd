"""The launch shape of the batched-inversion stages (kernels/inv_shape.hpp, used
by launch_chain for k_ec_scalar_batch and by launch_ed for k_ed_finish), read
through the test library: tokens per thread B = min(16, max(1, n / 131072)),
S = ceil(n / B) threads, one wave per block for an ECDSA launch of up to 16,384
tokens and four otherwise.  This pins which of the shapes of
test_gpu_ec_scalar_exact.py / test_gpu_ed_exact.py production runs at a given
launch size (host code only, but it lives in the device test library)."""
import ctypes
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#        n: (B, S, EC waves per block, EC grid, Ed grid)
TABLE = {
    64: (1, 64, 1, 1, 1),
    16384: (1, 16384, 1, 256, 64),
    16448: (1, 16448, 4, 65, 65),
    262080: (1, 262080, 4, 1024, 1024),
    262144: (2, 131072, 4, 512, 512),
    393216: (3, 131072, 4, 512, 512),
    1048576: (8, 131072, 4, 512, 512),
    2097088: (15, 139806, 4, 547, 547),
    2097152: (16, 131072, 4, 512, 512),
    4194304: (16, 262144, 4, 1024, 1024),
}


def _shape(fn, n):
    B, S, wpb, grid = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_uint()
    assert fn(ctypes.c_int64(n), ctypes.byref(B), ctypes.byref(S), ctypes.byref(wpb), ctypes.byref(grid)) == 0
    return B.value, S.value, wpb.value, grid.value


def test_launch_shape_table():
    tk = ctypes.CDLL(os.path.join(ROOT, "cap_amd", "libcapjwt_tk.so"))
    for n, (B, S, wpb, g_ec, g_ed) in TABLE.items():
        assert B == min(16, max(1, n // (256 * 8 * 64))) and S == -(-n // B)
        assert _shape(tk.tk_ec_scalar_shape, n) == (B, S, wpb, g_ec), n
        assert _shape(tk.tk_ed_finish_shape, n) == (B, S, 4, g_ed), n
        # every token has a thread, and no block is all idle
        for wp, g in ((wpb, g_ec), (4, g_ed)):
            assert (g - 1) * 64 * wp < S <= g * 64 * wp
    B = ctypes.c_int()
    for fn in (tk.tk_ec_scalar_shape, tk.tk_ed_finish_shape):
        assert fn(ctypes.c_int64(0), ctypes.byref(B), None, None, None) == -1
        assert fn(ctypes.c_int64(100), ctypes.byref(B), None, None, None) == -1
