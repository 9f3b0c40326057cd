// hash_operand.hpp -- the operand of a hash-claim predicate, made on the device.
//
// cap's oidc/id_token.go:121-145 (verifyHashClaim) holds at_hash / c_hash to
// base64.RawURLEncoding(h.Sum(nil)[:h.Size()/2]) of the access token or the
// authorization code, with sha256 / sha512.New384 / sha512 by the id_token's
// alg.  hash_operand() is that value for one source: it hashes the bytes with
// sha2.hpp's sha256_mem / sha512_mem (aligned word reads, as k_hash), takes the
// left half of the digest -- 16, 24 or 32 bytes -- and encodes it as 22, 32 or 43
// characters of unpadded base64url, four characters to a little-endian word,
// the bytes behind the last character zero.  The encoding runs on the digest
// words in registers with constant indices only (the loops unroll): no array is
// indexed at run time and nothing goes to scratch.
//
// Family 0 means "this job has no value" (an EdDSA id_token, a request without
// an access token).  Its operand is one byte, 0x00: a control byte inside a
// string sends the payload to the host (claims.hpp: c < 0x20 is `bad`), so no
// string the scan decides can equal it, and its length 1 keeps "" from matching.
//
// The function compiles for the host too (tests/host_kernels), so the CPU tests
// run the very code the kernel runs.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../../include/jg.h"
#include "sha2.hpp"

namespace jghop {

constexpr uint32_t kWords = 11;                 // an operand slot: 44 bytes, 43 characters at most
constexpr uint32_t kSlot = 4u * kWords;

// the base64url character of six bits, without a table
SHD uint32_t b64url_char(uint32_t v) {
  return v + 65u + (v >= 26u ? 6u : 0u) - (v >= 52u ? 75u : 0u) - (v >= 62u ? 13u : 0u) + (v >= 63u ? 49u : 0u);
}

// The operand of bytes [off, off + len) of `bytes` under family `fam` into w[0..11);
// returns its length in characters (1 for family 0).  Reads aligned words around
// the source as MemString does: the buffer carries slack behind it.
SHD uint32_t hash_operand(const uint8_t* bytes, uint32_t off, uint32_t len, uint32_t fam, uint32_t w[kWords]) {
#pragma unroll
  for (uint32_t k = 0; k < kWords; ++k) w[k] = 0u;
  if (fam == 0u) return 1u;                     // the byte 0x00
  sha2::MemString m;
  m.aligned = (const uint32_t*)(bytes + (off & ~3u));
  m.shift = off & 3u;
  m.len = len;
  uint32_t d[9];                                // the left half as big-endian words, zero behind it
#pragma unroll
  for (int k = 0; k < 9; ++k) d[k] = 0u;
  uint32_t nchar;
  if (fam == JG_SHA256) {
    uint32_t h[8];
    sha2::sha256_mem(h, m);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = h[k];
    nchar = 22u;
  } else {
    const bool is384 = fam == JG_SHA384;
    uint64_t h[8];
    sha2::sha512_mem(h, is384, m, nullptr, 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) { d[2 * k] = (uint32_t)(h[k] >> 32); d[2 * k + 1] = (uint32_t)h[k]; }
    d[6] = is384 ? 0u : (uint32_t)(h[3] >> 32);
    d[7] = is384 ? 0u : (uint32_t)h[3];
    nchar = is384 ? 32u : 43u;
  }
  // group j: digest bytes [3j, 3j + 3) -> characters [4j, 4j + 4) = word j
#pragma unroll
  for (uint32_t j = 0; j < kWords; ++j) {
    const uint32_t bit = 24u * j, wi = bit >> 5, sh = bit & 31u;          // constants once unrolled
    const uint64_t two = ((uint64_t)d[wi] << 32) | d[wi + 1u < 9u ? wi + 1u : 8u];
    const uint32_t t = (uint32_t)(two >> (40u - sh)) & 0xffffffu;
    const uint32_t c = b64url_char(t >> 18) | b64url_char((t >> 12) & 63u) << 8 | b64url_char((t >> 6) & 63u) << 16 |
                       b64url_char(t & 63u) << 24;
    const int rem = (int)nchar - (int)(4u * j);
    w[j] = rem >= 4 ? c : rem <= 0 ? 0u : c & ((1u << (8 * rem)) - 1u);
  }
  return nchar;
}

}  // namespace jghop

#if defined(__HIPCC__)
// One thread per (job, hash column): thread t = i * nhash + h hashes src[t] of
// src_bytes and stores the operand at op_bytes[op_base + 44 t, +44) and its span
// at spans[i * ncol + nstr + h], where k_claims_match_args reads string column
// nstr + h of job i.  op_base is a multiple of 4; every pointer is a device one.
void launch_hash_operand(const uint8_t* src_bytes, const jg_hsrc* src, int64_t njobs, uint32_t nhash, uint32_t nstr,
                         uint32_t op_base, uint8_t* op_bytes, jg_sarg* spans, hipStream_t s);
#endif
