// hash_operand.hip -- the operands of jg_claims_match_hash's EQUALS_HASH on gfx950.
//
// One thread per (job, hash column), 64 to a block as k_hash: it hashes the
// job's source (the access token, the authorization code), encodes the left
// half of the digest (hash_operand.hpp) and stores the characters and their
// span where k_claims_match_args, launched behind it on the same stream, reads
// that job's string operand.  The lanes of a wave may hold different families
// and lengths, so the SHA-256 and SHA-512 code and the block loops diverge; that
// cost is accepted (the sources are tens of bytes in the common case).
#include <hip/hip_runtime.h>

#include "hash_operand.hpp"

namespace {

__global__ void __launch_bounds__(64) k_hash_operand(const uint8_t* __restrict__ src_bytes,
                                                     const jg_hsrc* __restrict__ src, int64_t n, uint32_t nhash,
                                                     uint32_t nstr, uint32_t op_base, uint8_t* __restrict__ op_bytes,
                                                     jg_sarg* __restrict__ spans) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const jg_hsrc J = src[t];
  uint32_t w[jghop::kWords];
  const uint32_t nchar = jghop::hash_operand(src_bytes, J.off, J.len, J.fam, w);
  const uint32_t off = op_base + (uint32_t)t * jghop::kSlot;
  uint32_t* o = (uint32_t*)(op_bytes + off);
#pragma unroll
  for (uint32_t k = 0; k < jghop::kWords; ++k) o[k] = w[k];
  const int64_t i = t / nhash, h = t - i * nhash;
  *(uint2*)(spans + i * (nstr + nhash) + nstr + h) = make_uint2(off, nchar);
}

}  // namespace

void launch_hash_operand(const uint8_t* src_bytes, const jg_hsrc* src, int64_t njobs, uint32_t nhash, uint32_t nstr,
                         uint32_t op_base, uint8_t* op_bytes, jg_sarg* spans, hipStream_t s) {
  const int64_t n = njobs * nhash;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_hash_operand, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, src_bytes, src, n, nhash, nstr,
                     op_base, op_bytes, spans);
}
