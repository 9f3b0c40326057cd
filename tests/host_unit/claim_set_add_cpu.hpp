// jg_set_add's work on the CPU: the member check and the pool delta as the
// runtime makes them, and the steps of kernels/claim_set_insert.hpp with a
// sequential compare-and-swap, one "lane" after another.  Shared by
// claim_set_add_test.cpp and the stand-in ABI of tests/host_set_add.
#pragma once
#include <cstring>
#include <vector>

#include "../../cap_amd/csrc/kernels/claim_set_build.hpp"
#include "../../cap_amd/csrc/kernels/claim_set_insert.hpp"

namespace jgset {

// A table of 64-bit slot words with the accessors the steps take
struct SeqTable {
  std::vector<uint64_t> w;
  explicit SeqTable(size_t nslots) : w(nslots, 0) {}
  explicit SeqTable(const std::vector<Slot>& s) : w(s.size()) {
    for (size_t k = 0; k < s.size(); ++k) w[k] = slot_word(s[k].hash, s[k].ref);
  }
  auto load() {
    return [this](uint32_t i) -> uint64_t { return w.at(i); };
  }
  auto cas() {
    return [this](uint32_t i, uint64_t want) -> uint64_t {
      const uint64_t seen = w.at(i);
      if (!seen) w.at(i) = want;
      return seen;
    };
  }
  std::vector<Slot> slots() const {
    std::vector<Slot> s(w.size());
    for (size_t k = 0; k < w.size(); ++k) s[k] = Slot{(uint32_t)w[k], (uint32_t)(w[k] >> 32)};
    return s;
  }
};

// Adds members[k] = bytes[off, off + len), k < n, to *B in place.  0: done,
// *added of them were new.  -1: member *bad is refused (set_build's rule), *B
// untouched.  -2: a step found no slot, *B untouched.  -3: over 2^24 members.
inline int set_add_cpu(Built* B, const uint8_t* bytes, size_t bytes_len, const jg_sarg* members, size_t n,
                       uint32_t* added, size_t* bad) {
  for (size_t k = 0; k < n; ++k) {
    const jg_sarg& m = members[k];
    bool ok = m.len <= JG_SET_MEMBER_MAX && m.off <= bytes_len && m.len <= bytes_len - m.off;
    for (uint32_t b = 0; ok && b < m.len; ++b) ok = member_byte_ok(bytes[m.off + b]);
    if (!ok) {
      if (bad) *bad = k;
      return -1;
    }
  }
  if ((uint64_t)B->n + n > (uint64_t(1) << 24)) return -3;
  std::vector<uint32_t> pool(B->pool), refs(n);
  for (size_t k = 0; k < n; ++k) {
    const jg_sarg& m = members[k];
    const size_t at = pool.size();
    refs[k] = (uint32_t)at + 1u;
    pool.resize(at + 1u + (m.len + 3u) / 4u, 0u);
    pool[at] = m.len;
    for (uint32_t b = 0; b < m.len; ++b) pool[at + 1u + (b >> 2)] |= (uint32_t)bytes[m.off + b] << (8u * (b & 3u));
  }
  size_t nslots = B->slots.size();
  uint32_t maxprobe = B->maxprobe;
  SeqTable T(B->slots);
  if (2 * ((uint64_t)B->n + n) > nslots) {
    for (nslots = 1; nslots < 2 * ((uint64_t)B->n + n);) nslots *= 2;
    SeqTable G(nslots);
    maxprobe = 0;
    for (uint64_t s : T.w) {
      if (!s) continue;
      const uint32_t probe = set_rehash_step((uint32_t)nslots - 1u, s, G.load(), G.cas());
      if (!probe) return -2;
      maxprobe = probe > maxprobe ? probe : maxprobe;
    }
    T = G;
  }
  uint32_t placed = 0;
  for (size_t k = 0; k < n; ++k) {
    uint32_t probe = 0;
    const int r = set_insert_step(pool.data(), (uint32_t)nslots - 1u, set_entry_hash(pool.data(), refs[k], B->seed), refs[k],
                                  T.load(), T.cas(), &probe);
    if (r == kInsFull) return -2;
    if (r == kInsPlaced) {
      ++placed;
      maxprobe = probe > maxprobe ? probe : maxprobe;
    }
  }
  B->slots = T.slots();
  B->pool.swap(pool);
  B->maxprobe = maxprobe;
  B->n += placed;
  if (added) *added = placed;
  return 0;
}

}  // namespace jgset
