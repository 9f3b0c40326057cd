// claim_set.hpp -- resident sets of strings for the claims scan's set-membership
// predicates (JG_PRED_IN_SET, JG_PRED_ELEMENT_IN_SET).
//
// A set is immutable: an open-addressing table of 8-byte slots and a pool of
// dwords, built on the host from (members, seed) and read by any number of
// scans.  The layout, mirrored by tests/set_model.py:
//   slot   { hash, ref }: the member's finalised 32-bit hash and the index of its
//          pool entry plus one; ref 0 is an empty slot.  The slot count is a power
//          of two, at least twice the member count (1 for the empty set); a member
//          lies at the first free slot from hash & mask on, going up with
//          wrap-around, members taken in the order given (a repeated one folded
//          into its first occurrence).
//   entry  pool[ref - 1] is the length in bytes, 0..JG_SET_MEMBER_MAX, and the
//          next (length + 3) / 4 dwords are the bytes, little-endian, the last one
//          padded with zeros: a candidate is compared a dword at a time.
//   maxprobe  the longest run of slots any member's insertion looked at: the
//          trip bound of a lookup, so the loop does not depend on what it reads.
// The hash is byte-serial with 32 bits of state -- FNV-1a's xor-multiply from
// its usual basis, the same for every set, so a scan keeps one running hash of
// the open string however many sets it asks -- and is seeded where it is
// finalised: murmur3's mix of (state ^ seed), before it is masked to a slot.
// The seed moves a string's home slot and its stored hash from load to load; two
// strings of one state collide under every seed.  The hash only filters:
// set_probe confirms every hit byte for byte, so a collision costs a compare
// and never an answer.
// This header is what the kernels include: the layout, the hash and the lookup.
// set_build(), the host's half, is in claim_set_build.hpp.
#pragma once
#include <cstdint>

#include "../../../include/jg.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JG_SET_HD __host__ __device__ __forceinline__
#else
#define JG_SET_HD inline
#endif

namespace jgset {

struct Slot {
  uint32_t hash;
  uint32_t ref;               // the entry's dword in the pool + 1; 0: empty
};
static_assert(sizeof(Slot) == 8, "a slot is one 8-byte load");

// A built set as a lookup reads it
struct View {
  const Slot* slots;
  const uint32_t* pool;
  uint32_t mask;              // slots - 1
  uint32_t maxprobe;
  uint32_t seed;              // not read by set_probe: its caller finalises the hash with it (set_hash_final)
  uint32_t n;                 // distinct members; not read by a lookup: what jg_set_info reports travels with the view
};

JG_SET_HD uint32_t set_hash_step(uint32_t h, uint32_t c) { return (h ^ c) * 16777619u; }
constexpr uint32_t kHashBasis = 2166136261u;          // the state of the empty string
JG_SET_HD uint32_t set_hash_final(uint32_t h, uint32_t seed) {
  h ^= seed;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// Is the candidate of `len` bytes, whose finalised hash is h and whose byte i is
// cmp(i), a member of t?  cmp is only asked for i < len, in rising order.
template <class Cmp>
JG_SET_HD bool set_probe(const View& t, uint32_t h, uint32_t len, Cmp&& cmp) {
  uint32_t i = h & t.mask;
  for (uint32_t step = 0; step < t.maxprobe; ++step, i = (i + 1u) & t.mask) {
    const Slot s = t.slots[i];
    if (!s.ref) return false;
    if (s.hash != h) continue;
    const uint32_t* e = t.pool + (s.ref - 1u);
    if (e[0] != len) continue;
    bool same = true;
    for (uint32_t b = 0; same && b < len; b += 4u) {
      uint32_t v = 0;
      for (uint32_t k = 0; k < 4u; ++k) v |= b + k < len ? (cmp(b + k) & 0xffu) << (8u * k) : 0u;
      same = v == e[1u + (b >> 2)];
    }
    if (same) return true;
  }
  return false;
}

}  // namespace jgset
