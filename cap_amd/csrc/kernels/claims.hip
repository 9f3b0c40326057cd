// claims.hip -- batched scan of the registered claims on gfx950.
//
// The claim checks of cap's Validator.Validate after the signature
// (jwt/jwt.go:103-201) for callers that need the verdict only: one lane per
// token decodes the base64url payload segment and walks the JSON text with the
// scalar state machine of claims.hpp (claims_decide), reading the arena through
// aligned 32-bit words as hash.hip's MemString does -- one word load per four
// characters, never more than seven bytes past the segment (ARENA_SLACK covers
// it).  The resolved Expected (window edges, leeways, expected strings) is
// copied to LDS once per block; the byte compares of a claim value against the
// expected strings are LDS reads.  A wave runs until its longest payload ends.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "claims.hpp"

using namespace jgclaims;

namespace {

// characters [4g, 4g+4) of a segment that starts `shift` bytes into aligned[0]
struct WordSrc {
  const uint32_t* aligned;
  uint32_t shift8;            // 8 * (offset & 3)
  uint32_t cur;               // aligned[g]
  __device__ __forceinline__ uint32_t word(uint32_t g) {
    const uint32_t nxt = aligned[g + 1];
    const uint32_t w = (uint32_t)((((uint64_t)nxt << 32) | cur) >> shift8);
    cur = nxt;
    return w;
  }
};

constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) k_claims_scan(const uint8_t* __restrict__ arena,
                                                        const jg_cjob* __restrict__ jobs, int64_t n,
                                                        const Expect* __restrict__ expect,
                                                        uint8_t* __restrict__ code_out) {
  __shared__ Expect E;
  {
    static_assert(sizeof(Expect) % 4 == 0, "Expect is copied by words");
    const uint32_t* src = (const uint32_t*)expect;
    uint32_t* dst = (uint32_t*)&E;
    for (uint32_t k = threadIdx.x; k < sizeof(Expect) / 4; k += kBlock) dst[k] = src[k];
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const jg_cjob J = jobs[i];
  WordSrc src;
  src.aligned = (const uint32_t*)(arena + (J.off & ~(uint64_t)3));
  src.shift8 = 8u * (uint32_t)(J.off & 3);
  src.cur = src.aligned[0];
  code_out[i] = claims_decide(src, J.len, E);
}

// k_claims_scan that also keeps what it read: vals_out[i] is token i's record of
// registered claims (jg_claims, 64 bytes), written as four 16-byte stores
__global__ void __launch_bounds__(kBlock) k_claims_extract(const uint8_t* __restrict__ arena,
                                                           const jg_cjob* __restrict__ jobs, int64_t n,
                                                           const Expect* __restrict__ expect,
                                                           uint8_t* __restrict__ code_out,
                                                           jg_claims* __restrict__ vals_out) {
  __shared__ Expect E;
  {
    const uint32_t* src = (const uint32_t*)expect;
    uint32_t* dst = (uint32_t*)&E;
    for (uint32_t k = threadIdx.x; k < sizeof(Expect) / 4; k += kBlock) dst[k] = src[k];
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const jg_cjob J = jobs[i];
  WordSrc src;
  src.aligned = (const uint32_t*)(arena + (J.off & ~(uint64_t)3));
  src.shift8 = 8u * (uint32_t)(J.off & 3);
  src.cur = src.aligned[0];
  jg_claims v;                                  // fields only: stays in registers
  code_out[i] = claims_extract(src, J.len, E, &v);
  static_assert(sizeof(jg_claims) == 64, "the record is four 16-byte stores");
  uint4* o = (uint4*)(vals_out + i);
  o[0] = make_uint4((uint32_t)v.exp, (uint32_t)((uint64_t)v.exp >> 32), (uint32_t)v.nbf, (uint32_t)((uint64_t)v.nbf >> 32));
  o[1] = make_uint4((uint32_t)v.iat, (uint32_t)((uint64_t)v.iat >> 32), v.iss_off, v.iss_len);
  o[2] = make_uint4(v.sub_off, v.sub_len, v.jti_off, v.jti_len);
  o[3] = make_uint4(v.aud_off, v.aud_len, v.aud_n, v.present);
}

// k_claims_extract that also latches where the caller's named top-level
// members lie: sel_out[i] is token i's jg_selected (80 bytes), five 16-byte
// stores.  The resolved names sit in LDS beside the Expected; a depth-1 key is
// compared with them byte by byte from there.
__global__ void __launch_bounds__(kBlock) k_claims_select(const uint8_t* __restrict__ arena,
                                                          const jg_cjob* __restrict__ jobs, int64_t n,
                                                          const Expect* __restrict__ expect,
                                                          const Select* __restrict__ select,
                                                          uint8_t* __restrict__ code_out,
                                                          jg_claims* __restrict__ vals_out,
                                                          jg_selected* __restrict__ sel_out) {
  __shared__ Expect E;
  __shared__ Select S;
  {
    static_assert(sizeof(Select) % 4 == 0, "Select is copied by words");
    const uint32_t* src = (const uint32_t*)expect;
    uint32_t* dst = (uint32_t*)&E;
    for (uint32_t k = threadIdx.x; k < sizeof(Expect) / 4; k += kBlock) dst[k] = src[k];
    const uint32_t* ssrc = (const uint32_t*)select;
    uint32_t* sdst = (uint32_t*)&S;
    for (uint32_t k = threadIdx.x; k < sizeof(Select) / 4; k += kBlock) sdst[k] = ssrc[k];
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const jg_cjob J = jobs[i];
  WordSrc src;
  src.aligned = (const uint32_t*)(arena + (J.off & ~(uint64_t)3));
  src.shift8 = 8u * (uint32_t)(J.off & 3);
  src.cur = src.aligned[0];
  jg_claims v;                                  // fields and constant indices only: both stay in registers
  jg_selected q;
  code_out[i] = claims_select(src, J.len, E, S, &v, &q);
  uint4* o = (uint4*)(vals_out + i);
  o[0] = make_uint4((uint32_t)v.exp, (uint32_t)((uint64_t)v.exp >> 32), (uint32_t)v.nbf, (uint32_t)((uint64_t)v.nbf >> 32));
  o[1] = make_uint4((uint32_t)v.iat, (uint32_t)((uint64_t)v.iat >> 32), v.iss_off, v.iss_len);
  o[2] = make_uint4(v.sub_off, v.sub_len, v.jti_off, v.jti_len);
  o[3] = make_uint4(v.aud_off, v.aud_len, v.aud_n, v.present);
  static_assert(sizeof(jg_selected) == 80, "the record is five 16-byte stores");
  uint4* t = (uint4*)(sel_out + i);
  t[0] = make_uint4(q.off[0], q.off[1], q.off[2], q.off[3]);
  t[1] = make_uint4(q.off[4], q.off[5], q.off[6], q.off[7]);
  t[2] = make_uint4(q.len[0], q.len[1], q.len[2], q.len[3]);
  t[3] = make_uint4(q.len[4], q.len[5], q.len[6], q.len[7]);
  t[4] = make_uint4(q.type[0] | (uint32_t)q.type[1] << 8 | (uint32_t)q.type[2] << 16 | (uint32_t)q.type[3] << 24,
                    q.type[4] | (uint32_t)q.type[5] << 8 | (uint32_t)q.type[6] << 16 | (uint32_t)q.type[7] << 24, 0u, 0u);
}

// The three kernels above with a profile per lane (jg_claims_each): the block
// holds the call's Profiles table in LDS instead of one Expect, copied by words
// and only as far as it is in use -- the n headers (they follow the two counts)
// and the pool's used bytes, not all 16 KiB.  Lane i scans against header
// jobs[i].flags; the lanes of a wave may hold different profiles, which only
// makes the base of the LDS reads per-lane (their addresses depend on the lane's
// position in its value already).  M is the scan's mode; the records are
// written as above.  SL is what a selecting mode selects by: Select's names or,
// for kPath, Paths.
template <int M, class SL>
__device__ __forceinline__ void claims_each_body(Profiles& T, SL* S, const uint8_t* __restrict__ arena,
                                                 const jg_cjob* __restrict__ jobs, int64_t n,
                                                 const Profiles* __restrict__ table,
                                                 const SL* __restrict__ select, uint8_t* __restrict__ code_out,
                                                 jg_claims* __restrict__ vals_out, jg_selected* __restrict__ sel_out) {
  static_assert(offsetof(Profiles, h) == 8 && sizeof(ProfileHeader) % 4 == 0 && offsetof(Profiles, pool) % 4 == 0,
                "the table is copied by words");
  uint32_t np = table->n, used = table->pool_used;
  np = np < (uint32_t)JG_MAX_PROFILES ? np : (uint32_t)JG_MAX_PROFILES;       // the runtime resolved it: never taken
  used = used < (uint32_t)JG_PROFILE_POOL_BYTES ? used : (uint32_t)JG_PROFILE_POOL_BYTES;
  {
    const uint32_t* src = (const uint32_t*)table;
    uint32_t* dst = (uint32_t*)&T;
    const uint32_t hw = (8u + np * (uint32_t)sizeof(ProfileHeader)) / 4u;
    for (uint32_t k = threadIdx.x; k < hw; k += kBlock) dst[k] = src[k];
    constexpr uint32_t pw0 = offsetof(Profiles, pool) / 4u;
    const uint32_t pw = (used + 3u) / 4u;
    for (uint32_t k = threadIdx.x; k < pw; k += kBlock) dst[pw0 + k] = src[pw0 + k];
    if constexpr (M >= kSelect) {
      static_assert(sizeof(SL) % 4 == 0, "the names are copied by words");
      const uint32_t* ssrc = (const uint32_t*)select;
      uint32_t* sdst = (uint32_t*)S;
      for (uint32_t k = threadIdx.x; k < sizeof(SL) / 4; k += kBlock) sdst[k] = ssrc[k];
    }
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const jg_cjob J = jobs[i];
  const uint32_t p = J.flags < np ? J.flags : 0u;                             // likewise: checked before the launch
  WordSrc src;
  src.aligned = (const uint32_t*)(arena + (J.off & ~(uint64_t)3));
  src.shift8 = 8u * (uint32_t)(J.off & 3);
  src.cur = src.aligned[0];
  if constexpr (M == kVerdict) {
    code_out[i] = claims_decide_each(src, J.len, T, p);
  } else {
    jg_claims v;
    jg_selected q;
    if constexpr (M == kPath) code_out[i] = claims_paths_each(src, J.len, T, p, *S, &v, &q);
    else if constexpr (M == kSelect) code_out[i] = claims_select_each(src, J.len, T, p, *S, &v, &q);
    else code_out[i] = claims_extract_each(src, J.len, T, p, &v);
    uint4* o = (uint4*)(vals_out + i);
    o[0] = make_uint4((uint32_t)v.exp, (uint32_t)((uint64_t)v.exp >> 32), (uint32_t)v.nbf, (uint32_t)((uint64_t)v.nbf >> 32));
    o[1] = make_uint4((uint32_t)v.iat, (uint32_t)((uint64_t)v.iat >> 32), v.iss_off, v.iss_len);
    o[2] = make_uint4(v.sub_off, v.sub_len, v.jti_off, v.jti_len);
    o[3] = make_uint4(v.aud_off, v.aud_len, v.aud_n, v.present);
    if constexpr (M >= kSelect) {
      uint4* t = (uint4*)(sel_out + i);
      t[0] = make_uint4(q.off[0], q.off[1], q.off[2], q.off[3]);
      t[1] = make_uint4(q.off[4], q.off[5], q.off[6], q.off[7]);
      t[2] = make_uint4(q.len[0], q.len[1], q.len[2], q.len[3]);
      t[3] = make_uint4(q.len[4], q.len[5], q.len[6], q.len[7]);
      t[4] = make_uint4(q.type[0] | (uint32_t)q.type[1] << 8 | (uint32_t)q.type[2] << 16 | (uint32_t)q.type[3] << 24,
                        q.type[4] | (uint32_t)q.type[5] << 8 | (uint32_t)q.type[6] << 16 | (uint32_t)q.type[7] << 24, 0u, 0u);
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_claims_scan_each(const uint8_t* __restrict__ arena,
                                                             const jg_cjob* __restrict__ jobs, int64_t n,
                                                             const Profiles* __restrict__ table,
                                                             uint8_t* __restrict__ code_out) {
  __shared__ Profiles T;
  claims_each_body<kVerdict, Select>(T, nullptr, arena, jobs, n, table, nullptr, code_out, nullptr, nullptr);
}

__global__ void __launch_bounds__(kBlock) k_claims_extract_each(const uint8_t* __restrict__ arena,
                                                                const jg_cjob* __restrict__ jobs, int64_t n,
                                                                const Profiles* __restrict__ table,
                                                                uint8_t* __restrict__ code_out,
                                                                jg_claims* __restrict__ vals_out) {
  __shared__ Profiles T;
  claims_each_body<kExtract, Select>(T, nullptr, arena, jobs, n, table, nullptr, code_out, vals_out, nullptr);
}

__global__ void __launch_bounds__(kBlock) k_claims_select_each(const uint8_t* __restrict__ arena,
                                                               const jg_cjob* __restrict__ jobs, int64_t n,
                                                               const Profiles* __restrict__ table,
                                                               const Select* __restrict__ select,
                                                               uint8_t* __restrict__ code_out,
                                                               jg_claims* __restrict__ vals_out,
                                                               jg_selected* __restrict__ sel_out) {
  __shared__ Profiles T;
  __shared__ Select S;
  claims_each_body<kSelect, Select>(T, &S, arena, jobs, n, table, select, code_out, vals_out, sel_out);
}

// k_claims_select_each for members named by path (jg_claims_paths): the resolved
// paths sit in LDS beside the table, and a key at depth d <= JG_PATH_MAX_COMP is
// compared from there with component d of the paths matched that far.
__global__ void __launch_bounds__(kBlock) k_claims_paths_each(const uint8_t* __restrict__ arena,
                                                              const jg_cjob* __restrict__ jobs, int64_t n,
                                                              const Profiles* __restrict__ table,
                                                              const Paths* __restrict__ paths,
                                                              uint8_t* __restrict__ code_out,
                                                              jg_claims* __restrict__ vals_out,
                                                              jg_selected* __restrict__ sel_out) {
  __shared__ Profiles T;
  __shared__ Paths P;
  claims_each_body<kPath, Paths>(T, &P, arena, jobs, n, table, paths, code_out, vals_out, sel_out);
}

}  // namespace

void launch_claims_each(const uint8_t* arena, const jg_cjob* jobs, int64_t n, const Profiles* table,
                        const Select* select, uint8_t* code_out, jg_claims* vals_out, jg_selected* sel_out,
                        hipStream_t s) {
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
  if (sel_out)
    hipLaunchKernelGGL(k_claims_select_each, grid, block, 0, s, arena, jobs, n, table, select, code_out, vals_out,
                       sel_out);
  else if (vals_out)
    hipLaunchKernelGGL(k_claims_extract_each, grid, block, 0, s, arena, jobs, n, table, code_out, vals_out);
  else
    hipLaunchKernelGGL(k_claims_scan_each, grid, block, 0, s, arena, jobs, n, table, code_out);
}

void launch_claims_paths(const uint8_t* arena, const jg_cjob* jobs, int64_t n, const Profiles* table,
                         const Paths* paths, uint8_t* code_out, jg_claims* vals_out, jg_selected* sel_out,
                         hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_claims_paths_each, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, arena, jobs,
                     n, table, paths, code_out, vals_out, sel_out);
}

void launch_claims_select(const uint8_t* arena, const jg_cjob* jobs, int64_t n, const Expect* expect,
                          const Select* select, uint8_t* code_out, jg_claims* vals_out, jg_selected* sel_out,
                          hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_claims_select, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, arena, jobs, n,
                     expect, select, code_out, vals_out, sel_out);
}

void launch_claims_extract(const uint8_t* arena, const jg_cjob* jobs, int64_t n, const Expect* expect,
                           uint8_t* code_out, jg_claims* vals_out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_claims_extract, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, arena, jobs, n,
                     expect, code_out, vals_out);
}

void launch_claims_scan(const uint8_t* arena, const jg_cjob* jobs, int64_t n, const Expect* expect,
                        uint8_t* code_out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_claims_scan, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, arena, jobs, n,
                     expect, code_out);
}
