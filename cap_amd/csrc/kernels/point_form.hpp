// point_form.hpp -- which point kernel a launch of n padded tokens runs
// (launch_chain in ecdsa_impl.hpp, launch_ed in ed25519.hip): lanes per token,
// whether the lane's chain prefetches its table entries, and whether the
// one-lane kernel is the persistent k_ec_point.  Host-side and pure, so the
// test library can read the table back (tests/test_gpu_point_form.py).
#pragma once
#include <cstdint>

struct PointForm {
  int lanes;        // lanes per token: > 1 is k_ec_point_split / k_ed_point_split
  bool prefetch;    // one table entry ahead: k_ec_point_split<CV, S, true> / k_ed_point_pf
  bool persistent;  // k_ec_point taking 64-token groups from a counter, its grid capped
};

// the classes as common.hpp numbers them (ecdsa.hpp asserts it)
constexpr int PF_CLS_P256 = 4, PF_CLS_P384 = 5, PF_CLS_P521 = 6, PF_CLS_ED25519 = 7;

// The curves whose k_ec_point loops and takes the grid cap: P-256.  P-384
// measured no gain under the cap, so P-384 and P-521 keep
// one block per group and no counter.
constexpr bool ec_point_persistent(int cls) { return cls == PF_CLS_P256; }

// Launches of up to this many tokens run JG_EC_SPLIT lanes per token: under
// ~2 waves per SIMD the madd chain's latency is bare.
#ifndef JG_EC_SPLIT
#define JG_EC_SPLIT 4
#endif
#ifndef JG_EC_SPLIT_MAX
#define JG_EC_SPLIT_MAX 16384
#endif
// P-256 above that and up to this size: two lanes per token, prefetching (the
// second wave per SIMD hides more of the gather: DESIGN.md section 5, round 6).
#ifndef JG_EC_SPLIT2_P256
#define JG_EC_SPLIT2_P256 131072
#endif
// Up to this size (~1-4 waves per SIMD) one prefetching lane per token; above
// it k_ec_point and its four waves per SIMD.
#ifndef JG_EC_PF_MAX
#define JG_EC_PF_MAX 262144
#endif
// Launches of up to this many tokens: k_ec_scalar_batch<CV, 1>, one wave per
// block (inv_shape.hpp).
#ifndef JG_EC_SCALAR_SOLO_MAX
#define JG_EC_SCALAR_SOLO_MAX 16384
#endif
// Ed25519: JG_ED_SPLIT_LANES lanes per token up to JG_ED_SPLIT_MAX tokens; larger
// launches ran slower split.
#ifndef JG_ED_SPLIT_LANES
#define JG_ED_SPLIT_LANES 4
#endif
#ifndef JG_ED_SPLIT_MAX
#define JG_ED_SPLIT_MAX 16384
#endif
// Up to this size (under ~2 waves per SIMD) k_ed_point_pf, above it k_ed_point
// (DESIGN.md section 5, round 6).
#ifndef JG_ED_PF_MAX
#define JG_ED_PF_MAX 131072
#endif

constexpr int EC_SPLIT = JG_EC_SPLIT;                    // lanes per token of the small-launch split
constexpr int64_t EC_SPLIT_MAX_TOKENS = JG_EC_SPLIT_MAX;
constexpr int64_t EC_SPLIT2_MAX_P256 = JG_EC_SPLIT2_P256;
constexpr int64_t EC_PF_MAX_TOKENS = JG_EC_PF_MAX;
// P-521's prefetching chain takes 256 VGPRs (one wave per SIMD, 200 without):
// only launches of under ~one wave per SIMD
constexpr int64_t EC_PF_MAX_TOKENS_P521 = EC_PF_MAX_TOKENS < 65536 ? EC_PF_MAX_TOKENS : 65536;
constexpr int64_t EC_SCALAR_SOLO_MAX = JG_EC_SCALAR_SOLO_MAX;
constexpr int ED_SPLIT = JG_ED_SPLIT_LANES;
constexpr int64_t ED_SPLIT_MAX_TOKENS = JG_ED_SPLIT_MAX;
constexpr int64_t ED_PF_MAX_TOKENS = JG_ED_PF_MAX;
static_assert(EC_SPLIT == 2 || EC_SPLIT == 4, "the small-launch split is told from the one-lane rows by its lanes");
static_assert(ED_SPLIT == 2 || ED_SPLIT == 4, "two or four lanes per token");

// n: the padded tokens of the width run (a.end - a.begin).  force_point: the
// debugging switch EcArgs::force_point, k_ec_point at every size.
constexpr PointForm ec_point_form(int cls, int64_t n, bool force_point) {
  if (!force_point) {
    if (n <= EC_SPLIT_MAX_TOKENS) return {EC_SPLIT, false, false};
    if (cls == PF_CLS_P256 && n <= EC_SPLIT2_MAX_P256) return {2, true, false};
    if (n <= (cls == PF_CLS_P521 ? EC_PF_MAX_TOKENS_P521 : EC_PF_MAX_TOKENS)) return {1, true, false};
  }
  return {1, false, ec_point_persistent(cls)};
}

constexpr PointForm ed_point_form(int64_t n) {
  if (n <= ED_SPLIT_MAX_TOKENS) return {ED_SPLIT, false, false};
  if (n <= ED_PF_MAX_TOKENS) return {1, true, false};
  return {1, false, false};
}
