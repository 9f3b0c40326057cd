// tk_claim_set_insert.hip -- TEST INFRASTRUCTURE (libcapjwt_tk.so only, never
// the product path): k_set_rehash and k_set_insert (kernels/claim_set_insert.hip)
// alone, through their production launchers, on a table and a pool the caller
// hands in, so tests/test_gpu_set_insert.py can check the resulting table with
// tests/set_add_model.py without a context around it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../kernels/claim_set_insert.hip"

// old_slots: old_nslots (hash, ref) pairs, the table before.  pool: pool_dwords
// dwords, the old pool with the new entries packed behind it.  refs[k], k < n:
// the entries to insert (dword index + 1).  new_nslots == old_nslots: the table
// is copied and the insert starts from old_maxprobe; larger: the new table is
// zeroed, k_set_rehash moves the old slots and the insert starts from its
// maxprobe.  slots_out: new_nslots pairs; pool_out: pool_dwords dwords as they
// lie on the device after the launches; words_out: added, maxprobe, error.
// Returns 0; -1, with nothing launched, for input the kernels could leave their
// buffers on or spin over: slot counts that are no powers of two or shrink, a
// pool that is not a run of well-formed entries (length at most
// JG_SET_MEMBER_MAX) end to end, a ref of a slot or of refs[] that is not the
// start of one, or more than new_nslots / 2 occupied slots and refs together
// (one slot is enough for none); -2 on a HIP error.
extern "C" int tk_set_insert(const uint32_t* old_slots, uint32_t old_nslots, uint32_t new_nslots, const uint32_t* pool,
                             uint32_t pool_dwords, const uint32_t* refs, uint32_t n, uint32_t old_maxprobe,
                             uint32_t seed, uint32_t* slots_out, uint32_t* pool_out, uint32_t* words_out) {
  if (!old_slots || old_nslots == 0 || (old_nslots & (old_nslots - 1u)) || new_nslots < old_nslots ||
      (new_nslots & (new_nslots - 1u)) || new_nslots > (1u << 25) || old_maxprobe > old_nslots ||
      (pool_dwords && !pool) || pool_dwords > (1u << 27) || (n && !refs) || n > (1u << 24) || !slots_out ||
      (pool_dwords && !pool_out) || !words_out)
    return -1;
  std::vector<bool> start(pool_dwords + 1u, false);
  uint64_t at = 0;
  while (at < pool_dwords) {
    if (pool[at] > JG_SET_MEMBER_MAX) return -1;
    start[at] = true;
    at += 1u + (pool[at] + 3u) / 4u;
  }
  if (at != pool_dwords) return -1;
  uint64_t occupied = 0;
  for (uint32_t k = 0; k < old_nslots; ++k) {
    const uint32_t ref = old_slots[2 * k + 1];
    if (!ref) continue;
    ++occupied;
    if (ref > pool_dwords || !start[ref - 1u]) return -1;
  }
  for (uint32_t k = 0; k < n; ++k)
    if (!refs[k] || refs[k] > pool_dwords || !start[refs[k] - 1u]) return -1;
  if (occupied + n > 0 && 2 * (occupied + n) > new_nslots) return -1;
  jgset::Slot *dold = nullptr, *dnew = nullptr;
  uint32_t *dp = nullptr, *dr = nullptr;
  jgset::InsertWords* dw = nullptr;
  const bool grow = new_nslots != old_nslots;
  int rc = -2;
  do {
    if (hipMalloc(&dold, sizeof(jgset::Slot) * old_nslots) != hipSuccess) break;
    if (hipMalloc(&dnew, sizeof(jgset::Slot) * new_nslots) != hipSuccess) break;
    if (hipMalloc(&dp, 4 * (size_t)pool_dwords + 16) != hipSuccess) break;
    if (hipMalloc(&dr, 4 * (size_t)n + 16) != hipSuccess) break;
    if (hipMalloc(&dw, sizeof(jgset::InsertWords)) != hipSuccess) break;
    if (hipMemcpy(dold, old_slots, sizeof(jgset::Slot) * old_nslots, hipMemcpyHostToDevice) != hipSuccess) break;
    if (pool_dwords && hipMemcpy(dp, pool, 4 * (size_t)pool_dwords, hipMemcpyHostToDevice) != hipSuccess) break;
    if (n && hipMemcpy(dr, refs, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) break;
    const jgset::InsertWords w0{0u, grow ? 0u : old_maxprobe, 0u};
    if (hipMemcpy(dw, &w0, sizeof w0, hipMemcpyHostToDevice) != hipSuccess) break;
    if (grow) {
      if (hipMemset(dnew, 0, sizeof(jgset::Slot) * new_nslots) != hipSuccess) break;
      if (jgset::launch_set_rehash(dold, old_nslots, dnew, new_nslots, dw, nullptr) != hipSuccess) break;
    } else if (hipMemcpy(dnew, dold, sizeof(jgset::Slot) * old_nslots, hipMemcpyDeviceToDevice) != hipSuccess) {
      break;
    }
    if (jgset::launch_set_insert(dnew, new_nslots, dp, dr, n, seed, dw, nullptr) != hipSuccess) break;
    if (hipDeviceSynchronize() != hipSuccess) break;
    if (hipMemcpy(slots_out, dnew, sizeof(jgset::Slot) * new_nslots, hipMemcpyDeviceToHost) != hipSuccess) break;
    if (pool_dwords && hipMemcpy(pool_out, dp, 4 * (size_t)pool_dwords, hipMemcpyDeviceToHost) != hipSuccess) break;
    if (hipMemcpy(words_out, dw, sizeof(jgset::InsertWords), hipMemcpyDeviceToHost) != hipSuccess) break;
    rc = 0;
  } while (false);
  (void)hipFree(dold);
  (void)hipFree(dnew);
  (void)hipFree(dp);
  (void)hipFree(dr);
  (void)hipFree(dw);
  return rc;
}
