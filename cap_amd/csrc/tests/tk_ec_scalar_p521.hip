// tk_ec_scalar_p521.hip -- TEST INFRASTRUCTURE (libcapjwt_tk.so only): the
// P-521 instantiations of k_ec_scalar_batch for the tk_ec_scalar hook, capped
// at two waves per SIMD as kernels/ecdsa_p521.hip compiles them.
#define JG_EC_SCALAR_ATTR __attribute__((amdgpu_waves_per_eu(2)))
#include "tk_ec_scalar.hpp"

bool tkes_launch_p521(int wq, int wpb, const EcArgs& a, int B) {
  if (wpb == EC_SCALAR_WPB) {
    if (wq == 20) tkes_launch<CurveP521W<20>, EC_SCALAR_WPB>(a, B);
    else if (wq == 18) tkes_launch<CurveP521W<18>, EC_SCALAR_WPB>(a, B);
    else if (wq == 16) tkes_launch<CurveP521W<16>, EC_SCALAR_WPB>(a, B);
    else return false;
    return true;
  }
  if (wpb == 1 && wq == 16) {
    tkes_launch<CurveP521W<16>, 1>(a, B);
    return true;
  }
  return false;
}
