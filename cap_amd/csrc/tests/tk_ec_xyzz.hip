// tk_ec_xyzz.hip -- the addition chain of k_ec_point on the XYZZ accumulator,
// on caller-supplied points (test infrastructure: built into libcapjwt_tk.so,
// used only by tests/test_gpu_ec_xyzz_exact.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../kernels/ecdsa_impl.hpp"

namespace {

// Lane i adds its first cnt[i] of `steps` points with ec_point_token's calls:
// step 0 and steps >= 2 through add_ent<CV, false, true>, step 1 through
// add_ent<CV, true, true> (the peeled Q entry of window 0, onto ZZ == 1).
// A step of sign 0 adds nothing, as a zero digit.
template <class CV>
__global__ void __launch_bounds__(64) k_tk_xyzz_chain(const uint32_t* pts, const int32_t* sign, const int32_t* cnt,
                                                      uint32_t* out, int n, int steps) {
  using Fp = typename CV::Fp;
  constexpr int L = Fp::L;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = cnt[i] < steps ? cnt[i] : steps;
  uint32_t X[L], Y[L], ZZ[L], ZZZ[L];
#pragma unroll
  for (int j = 0; j < L; ++j) X[j] = Y[j] = ZZ[j] = ZZZ[j] = 0;
  bool empty = true;
  auto ent = [&](int s, RawEnt<CV>& r) {
    const uint32_t* p = pts + ((size_t)i * steps + s) * 2 * L;
    uint32_t x[L], y[L];
#pragma unroll
    for (int j = 0; j < L; ++j) { x[j] = p[j]; y[j] = p[L + j]; }
    store_entry<CV>(r.w, x, y);              // the table's entry format, as load_ent leaves it
    return sign[(size_t)i * steps + s];
  };
  RawEnt<CV> r;
  if (c > 0) { const int d = ent(0, r); add_ent<CV, false, true>(X, Y, ZZ, empty, r, d, ZZZ); }
  if (c > 1) { const int d = ent(1, r); add_ent<CV, true, true>(X, Y, ZZ, empty, r, d, ZZZ); }
#pragma unroll 1
  for (int s = 2; s < c; ++s) {
    const int d = ent(s, r);
    add_ent<CV, false, true>(X, Y, ZZ, empty, r, d, ZZZ);
  }
  uint32_t* o = out + (size_t)i * (4 * L + 1);
#pragma unroll
  for (int j = 0; j < L; ++j) { o[j] = X[j]; o[L + j] = Y[j]; o[2 * L + j] = ZZ[j]; o[3 * L + j] = ZZZ[j]; }
  o[4 * L] = empty ? 1u : 0u;
}

template <class CV>
int run_chain(const uint32_t* pts, const int32_t* sign, const int32_t* cnt, uint32_t* out, int n, int steps) {
  if constexpr (!ec_point_xyzz(CV::CLS)) {
    return -1;                                // the curve's k_ec_point is Jacobian
  } else {
    constexpr int L = CV::Fp::L;
    if (n <= 0 || steps <= 0) return -1;
    const size_t pb = sizeof(uint32_t) * 2 * L * (size_t)n * steps, sb = sizeof(int32_t) * (size_t)n * steps,
                 cb = sizeof(int32_t) * (size_t)n, ob = sizeof(uint32_t) * (4 * L + 1) * (size_t)n;
    void *dp = nullptr, *ds = nullptr, *dc = nullptr, *dout = nullptr;
    if (hipMalloc(&dp, pb) || hipMalloc(&ds, sb) || hipMalloc(&dc, cb) || hipMalloc(&dout, ob)) return -1;
    (void)hipMemcpy(dp, pts, pb, hipMemcpyHostToDevice);
    (void)hipMemcpy(ds, sign, sb, hipMemcpyHostToDevice);
    (void)hipMemcpy(dc, cnt, cb, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_tk_xyzz_chain<CV>, dim3((n + 63) / 64), dim3(64), 0, 0, (const uint32_t*)dp,
                       (const int32_t*)ds, (const int32_t*)dc, (uint32_t*)dout, n, steps);
    const hipError_t e = hipDeviceSynchronize();
    (void)hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
    (void)hipFree(dp); (void)hipFree(ds); (void)hipFree(dc); (void)hipFree(dout);
    return e == hipSuccess ? 0 : -2;
  }
}

}  // namespace

// curve: 1 P-256, 2 P-384, 3 P-521 (-1 for a curve whose k_ec_point is not on
// the XYZZ accumulator).  pts: n x steps x (x, y) canonical Montgomery 28-bit
// limbs, lane-major; sign: n x steps of +1 / -1 / 0; cnt: n step counts;
// out: n x (X, Y, ZZ, ZZZ limbs, then 1 if nothing was added).
extern "C" int tk_ec_xyzz_chain(int curve, const uint32_t* pts, const int32_t* sign, const int32_t* cnt,
                                uint32_t* out, int n, int steps) {
  switch (curve) {
    case 1: return run_chain<CurveP256>(pts, sign, cnt, out, n, steps);
    case 2: return run_chain<CurveP384>(pts, sign, cnt, out, n, steps);
    case 3: return run_chain<CurveP521>(pts, sign, cnt, out, n, steps);
    default: return -1;
  }
}
