// claim_set_insert.hip -- the kernels behind jg_set_add:
// k_set_rehash moves a table's slots into a larger one, k_set_insert places new
// pool entries.  The steps themselves are claim_set_insert.hpp's.
//
// Memory model.  Lanes of different workgroups, on different XCDs, race for one
// slot.  Every access to a slot here is a 64-bit agent-scope atomic on a global
// (address space 1) pointer -- a relaxed load or a compare-and-swap against 0 --
// never a plain or flat load, which a CU's L1 could serve from a stale line.
// Relaxed ordering is enough: a slot word is self-contained (hash and ref travel
// in the one word that is swapped in), and what its ref names, the pool, was
// written whole by the copies in front of the launch on the same stream; no lane
// of a launch writes a byte another lane reads other than through these atomics.
#include <hip/hip_runtime.h>

#include "claim_set_insert.hpp"

namespace jgset {
namespace {

typedef __attribute__((address_space(1))) unsigned long long gu64;

struct SlotLoad {
  gu64* t;
  __device__ uint64_t operator()(uint32_t i) const {
    return __hip_atomic_load(t + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};
struct SlotCas {
  gu64* t;
  __device__ uint64_t operator()(uint32_t i, uint64_t want) const {
    unsigned long long seen = 0;
    __hip_atomic_compare_exchange_strong(t + i, &seen, (unsigned long long)want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    return seen;                 // 0: swapped in; otherwise what the slot held
  }
};

// The wave's largest v in every lane (all 64 lanes take part)
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

// One lane per old slot.  No member bytes are read: the slot holds the hash.
__global__ void __launch_bounds__(256) k_set_rehash(const Slot* old_slots, uint32_t old_nslots, Slot* new_slots,
                                                    uint32_t newmask, InsertWords* words) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  gu64* told = (gu64*)(unsigned long long*)old_slots;
  gu64* tnew = (gu64*)(unsigned long long*)new_slots;
  uint32_t probe = 0;
  bool lost = false;
  if (i < old_nslots) {
    const uint64_t s = SlotLoad{told}(i);
    if (s) {
      probe = set_rehash_step(newmask, s, SlotLoad{tnew}, SlotCas{tnew});
      lost = probe == 0;
    }
  }
  if (lost) atomicOr(&words->error, 1u);
  const uint32_t wmax = wave_max(probe);
  if ((threadIdx.x & 63u) == 0 && wmax) atomicMax(&words->maxprobe, wmax);
}

// One lane per new entry
__global__ void __launch_bounds__(256) k_set_insert(Slot* slots, uint32_t mask, const uint32_t* pool,
                                                    const uint32_t* refs, uint32_t n, uint32_t seed,
                                                    InsertWords* words) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  gu64* t = (gu64*)(unsigned long long*)slots;
  uint32_t probe = 0;
  int r = kInsDuplicate;
  if (i < n) {
    const uint32_t ref = refs[i];
    r = set_insert_step(pool, mask, set_entry_hash(pool, ref, seed), ref, SlotLoad{t}, SlotCas{t}, &probe);
  }
  if (r == kInsPlaced) atomicAdd(&words->added, 1u);
  if (r == kInsFull) atomicOr(&words->error, 2u);
  const uint32_t wmax = wave_max(probe);
  if ((threadIdx.x & 63u) == 0 && wmax) atomicMax(&words->maxprobe, wmax);
}

}  // namespace

hipError_t launch_set_rehash(const Slot* old_slots, uint32_t old_nslots, Slot* new_slots, uint32_t new_nslots,
                             InsertWords* words, hipStream_t stream) {
  hipLaunchKernelGGL(k_set_rehash, dim3((old_nslots + 255u) / 256u), dim3(256), 0, stream, old_slots, old_nslots,
                     new_slots, new_nslots - 1u, words);
  return hipGetLastError();
}

hipError_t launch_set_insert(Slot* slots, uint32_t nslots, const uint32_t* pool, const uint32_t* refs, uint32_t n,
                             uint32_t seed, InsertWords* words, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_set_insert, dim3((n + 255u) / 256u), dim3(256), 0, stream, slots, nslots - 1u, pool, refs, n,
                     seed, words);
  return hipGetLastError();
}

}  // namespace jgset
