// claim_set_insert.hpp -- adding members to a resident set (jg_set_add; DESIGN.md
// 10.10): the step that places one pool entry in a table, and the step that
// moves one slot of a table into a larger one.  Both are __host__ __device__ with
// the slot accessors passed in, as set_probe takes its compare: the kernels of
// claim_set_insert.hip hand them agent-scope atomics, and the CPU program under
// tests/host_unit compiles the same code with a sequential compare-and-swap.
//
// A slot is read and written as one 64-bit word, hash in the low half and ref in
// the high half (Slot's bytes, little-endian); 0 is the empty slot, and no
// occupied slot is 0 because its ref is not.  A slot only ever changes from 0 to
// its final value, so a word that was read non-zero stays what it was.
#pragma once
#include <cstdint>

#include "claim_set.hpp"

namespace jgset {

JG_SET_HD uint64_t slot_word(uint32_t hash, uint32_t ref) { return (uint64_t)ref << 32 | hash; }

// What set_insert_step did with its entry
enum : int {
  kInsPlaced = 0,                // it has a slot now: *probe slots were looked at, its own included
  kInsDuplicate = 1,             // an equal entry has one: resident before, or placed by another lane of this launch
  kInsFull = 2,                  // nslots slots looked at, none empty and none equal: the table is full (an error)
};

// The finalised hash of the entry at pool[ref - 1], from its dwords
JG_SET_HD uint32_t set_entry_hash(const uint32_t* pool, uint32_t ref, uint32_t seed) {
  const uint32_t* e = pool + (ref - 1u);
  const uint32_t len = e[0];
  uint32_t h = kHashBasis;
  for (uint32_t b = 0; b < len; b += 4u) {
    const uint32_t v = e[1u + (b >> 2)];
    for (uint32_t k = 0; k < 4u && b + k < len; ++k) h = set_hash_step(h, (v >> (8u * k)) & 0xffu);
  }
  return set_hash_final(h, seed);
}

// Places the entry `ref` of hash h in the table of mask + 1 slots.
//   load(i)         the word of slot i
//   cas(i, want)    stores `want` in slot i if it holds 0; returns what it held
// A lost compare-and-swap looks at the same slot again: the winner may be an
// equal entry.  The trip count is bounded by the slot count, not by what is read.
template <class Load, class Cas>
JG_SET_HD int set_insert_step(const uint32_t* pool, uint32_t mask, uint32_t h, uint32_t ref, Load&& load, Cas&& cas,
                              uint32_t* probe) {
  const uint32_t* mine = pool + (ref - 1u);
  const uint32_t len = mine[0], words = (len + 3u) / 4u;
  const uint64_t want = slot_word(h, ref);
  uint32_t i = h & mask;
  for (uint32_t step = 0; step <= mask; ++step, i = (i + 1u) & mask) {
    uint64_t s = load(i);
    if (!s) {
      s = cas(i, want);
      if (!s) {
        *probe = step + 1u;
        return kInsPlaced;
      }
    }
    if ((uint32_t)s != h) continue;
    const uint32_t* e = pool + ((uint32_t)(s >> 32) - 1u);
    if (e[0] != len) continue;
    bool same = true;
    for (uint32_t w = 0; same && w < words; ++w) same = e[1u + w] == mine[1u + w];
    if (same) return kInsDuplicate;
  }
  return kInsFull;
}

// Moves the occupied slot word s of an old table to the first empty slot of the
// new one from its hash's home on.  Returns the slots looked at, 0 when the new
// table had no empty slot (an error: it is at least as large as the old one).
template <class Load, class Cas>
JG_SET_HD uint32_t set_rehash_step(uint32_t newmask, uint64_t s, Load&& load, Cas&& cas) {
  uint32_t i = (uint32_t)s & newmask;
  for (uint32_t step = 0; step <= newmask; ++step, i = (i + 1u) & newmask)
    if (!load(i) && !cas(i, s)) return step + 1u;
  return 0;
}

// The three words a launch reports, zeroed (maxprobe: set to the old set's) in front of it
struct InsertWords {
  uint32_t added, maxprobe, error;
};

#if defined(__HIPCC__)
// Both launch on `stream` and return the launch's status; nothing is waited for.
// old_slots / new_slots: tables of old_nslots / new_nslots slots (powers of two,
// new >= old), the new one zeroed; words->maxprobe 0.
hipError_t launch_set_rehash(const Slot* old_slots, uint32_t old_nslots, Slot* new_slots, uint32_t new_nslots,
                             InsertWords* words, hipStream_t stream);
// refs[k], k < n: the entries to place, all inside pool, which is complete.
hipError_t launch_set_insert(Slot* slots, uint32_t nslots, const uint32_t* pool, const uint32_t* refs, uint32_t n,
                             uint32_t seed, InsertWords* words, hipStream_t stream);
#endif

}  // namespace jgset
