// inv_shape.hpp -- launch shape of the batched-inversion stages
// (k_ec_scalar_batch in ecdsa_impl.hpp, k_ed_finish in ed25519.hip): thread i
// of the launch owns the B tokens begin + i + j S, j < B, and the waves of a
// block share one inversion (mp::block_inv).
#pragma once
#include <cstdint>

struct InvShape {
  int B;            // tokens per thread
  int64_t S;        // threads with work = stride between a thread's tokens: ceil(n / B)
  int wpb;          // waves per block
  unsigned grid;    // blocks of 64 wpb threads covering S
};

// n: padded tokens of the launch.  Tokens per thread keep >= ~8 waves per CU
// (256 CUs: profiles/r04_s3/scalar_occupancy_ab.json -- more waves and fewer
// tokens per inversion measured 12-26 % slower), 16 at the most.  Launches of
// up to solo_max tokens run one wave per block (one inversion per wave, no
// block barrier: the shared inversion saves inversions only when the chip is
// full); larger ones wpb_full waves.
constexpr InvShape inv_shape(int64_t n, int wpb_full, int64_t solo_max) {
  constexpr int64_t wpc = 8, cus = 256, wave = 64;
  const int64_t q = n / (cus * wpc * wave);
  const int B = (int)(q < 1 ? 1 : q > 16 ? 16 : q);
  const int64_t S = (n + B - 1) / B;
  const int wpb = n <= solo_max ? 1 : wpb_full;
  const int64_t tpb = wave * wpb;
  return InvShape{B, S, wpb, (unsigned)((S + tpb - 1) / tpb)};
}
