// tk_ec_scalar.hpp -- TEST INFRASTRUCTURE (libcapjwt_tk.so only): what the
// translation units of the tk_ec_scalar hook share.  tk_ec_scalar.hip holds the
// hook and the P-256 / P-384 instantiations of k_ec_scalar_batch;
// tk_ec_scalar_p521.hip the P-521 ones, compiled with the occupancy attribute
// of kernels/ecdsa_p521.hip.
#pragma once
#include "../kernels/ecdsa_impl.hpp"

namespace {

// k_ec_scalar_batch<CV, WPB> with launch_chain's grid and block for B tokens
// per thread: blocks of 64 WPB threads covering S = ceil(n / B) threads
template <class CV, int WPB>
void tkes_launch(const EcArgs& a, int B) {
  const int64_t n = a.end - a.begin, S = (n + B - 1) / B;
  constexpr int TPB = WAVE * WPB;
  hipLaunchKernelGGL((k_ec_scalar_batch<CV, WPB>), dim3((unsigned)((S + TPB - 1) / TPB)), dim3(TPB), 0, 0, a, B);
}

}  // namespace

// false: no such instantiation (nothing launched).  Every key width with WPB =
// EC_SCALAR_WPB, the curve's narrowest width with WPB = 1 as well.
bool tkes_launch_p256(int wq, int wpb, const EcArgs& a, int B);
bool tkes_launch_p384(int wq, int wpb, const EcArgs& a, int B);
bool tkes_launch_p521(int wq, int wpb, const EcArgs& a, int B);
