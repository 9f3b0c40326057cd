// claim_set_build.hpp -- the host's half of claim_set.hpp: set_build(), which
// makes the table and the pool of a resident set from (members, seed).  Kept out
// of claim_set.hpp so that the kernels' translation units do not pull in the
// containers it uses; included by the runtime (jg_set_load) and by the host
// programs under tests/host_unit.
#pragma once
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "claim_set.hpp"

namespace jgset {

// A member's byte as the device compares it: a predicate value's byte (claims.hpp name_byte_ok)
inline bool member_byte_ok(uint8_t c) { return c >= 0x20u && c <= 0x7eu && c != '"' && c != '\\'; }

// set_build's result: what is uploaded, and the numbers jg_set_info reports
struct Built {
  std::vector<Slot> slots;
  std::vector<uint32_t> pool;
  uint32_t n = 0, maxprobe = 0, seed = 0;
  View view() const { return View{slots.data(), pool.data(), (uint32_t)slots.size() - 1u, maxprobe, seed, n}; }
};

// Builds the set of members[k] = bytes[off, off + len), k < n, under `seed`.
// 0: built.  -1: member *bad is refused -- a span past bytes_len, over
// JG_SET_MEMBER_MAX bytes, or a byte member_byte_ok() refuses.  -3: over 2^24
// distinct members or a pool of 2^32 bytes or more (*bad untouched).  The result
// is a function of the distinct members in their order and of the seed alone.
inline int set_build(const uint8_t* bytes, size_t bytes_len, const jg_sarg* members, size_t n, uint32_t seed,
                     Built* out, size_t* bad) {
  std::unordered_set<std::string> seen;
  std::vector<size_t> keep;
  uint64_t dwords = 0;
  for (size_t k = 0; k < n; ++k) {
    const jg_sarg& m = members[k];
    bool ok = m.len <= JG_SET_MEMBER_MAX && m.off <= bytes_len && m.len <= bytes_len - m.off;
    for (uint32_t b = 0; ok && b < m.len; ++b) ok = member_byte_ok(bytes[m.off + b]);
    if (!ok) {
      if (bad) *bad = k;
      return -1;
    }
    if (!seen.emplace(m.len ? (const char*)bytes + m.off : "", m.len).second) continue;
    keep.push_back(k);
    dwords += 1u + (m.len + 3u) / 4u;
  }
  if (keep.size() > (size_t(1) << 24) || dwords * 4u >= (uint64_t(1) << 32)) return -3;
  size_t nslots = 1;
  while (nslots < 2 * keep.size()) nslots *= 2;
  out->slots.assign(nslots, Slot{0u, 0u});
  out->pool.assign((size_t)dwords, 0u);
  out->n = (uint32_t)keep.size();
  out->seed = seed;
  out->maxprobe = 0;
  const uint32_t mask = (uint32_t)nslots - 1u;
  uint32_t at = 0;
  for (size_t k : keep) {
    const jg_sarg& m = members[k];
    uint32_t h = kHashBasis;
    for (uint32_t b = 0; b < m.len; ++b) h = set_hash_step(h, bytes[m.off + b]);
    h = set_hash_final(h, seed);
    out->pool[at] = m.len;
    for (uint32_t b = 0; b < m.len; ++b) out->pool[at + 1u + (b >> 2)] |= (uint32_t)bytes[m.off + b] << (8u * (b & 3u));
    uint32_t i = h & mask, probe = 1;
    while (out->slots[i].ref) {
      i = (i + 1u) & mask;
      ++probe;
    }
    out->slots[i] = Slot{h, at + 1u};
    out->maxprobe = probe > out->maxprobe ? probe : out->maxprobe;
    at += 1u + (m.len + 3u) / 4u;
  }
  return 0;
}

}  // namespace jgset
