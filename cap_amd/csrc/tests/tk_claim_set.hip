// tk_claim_set.hip -- TEST INFRASTRUCTURE (libcapjwt_tk.so only, never the
// product path): set_probe (kernels/claim_set.hpp) alone on the device, one lane
// per query string, against a table the caller hands in as set_model.py or
// set_build() made it, so tests/test_gpu_set_probe.py can compare every answer
// with Python's `in` -- the scan around it only ever asks about strings a payload
// happens to hold.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../kernels/claim_set.hpp"

namespace {

__global__ void __launch_bounds__(256) k_tk_set_probe(jgset::View t, const uint8_t* __restrict__ qbytes,
                                                      const jg_sarg* __restrict__ q, int64_t nq,
                                                      uint8_t* __restrict__ hit_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nq) return;
  const uint8_t* p = qbytes + q[i].off;
  const uint32_t len = q[i].len;
  uint32_t h = jgset::kHashBasis;
  for (uint32_t b = 0; b < len; ++b) h = jgset::set_hash_step(h, p[b]);
  hit_out[i] = jgset::set_probe(t, jgset::set_hash_final(h, t.seed), len, [p](uint32_t b) -> uint32_t { return p[b]; }) ? 1 : 0;
}

}  // namespace

// slots: nslots (hash, ref) pairs; pool: pool_dwords dwords; q: nq spans of
// qbytes.  hit_out[i] = 1 when query i is a member, else 0 (poisoned with 0xA5
// before the launch).  Returns 0; -1 for a table or queries a lookup could leave
// its buffers on (the kernel is not launched): a slot count that is no power of
// two, maxprobe over it, a ref whose entry does not lie in the pool with a
// length of at most JG_SET_MEMBER_MAX, a query span past qbytes_len; -2 on a HIP
// error.
extern "C" int tk_set_probe(const uint32_t* slots, uint32_t nslots, const uint32_t* pool, uint32_t pool_dwords,
                            uint32_t maxprobe, uint32_t seed, const uint8_t* qbytes, uint64_t qbytes_len,
                            const jg_sarg* q, int64_t nq, uint8_t* hit_out) {
  if (!slots || nslots == 0 || (nslots & (nslots - 1u)) || nslots > (1u << 25) || maxprobe > nslots ||
      (pool_dwords && !pool) || nq <= 0 || nq > (1 << 20) || !q || !hit_out || (qbytes_len && !qbytes) ||
      qbytes_len >= (uint64_t(1) << 31))
    return -1;
  uint32_t n = 0;
  for (uint32_t k = 0; k < nslots; ++k) {
    const uint32_t ref = slots[2 * k + 1];
    if (!ref) continue;
    ++n;
    if (ref > pool_dwords || pool[ref - 1u] > JG_SET_MEMBER_MAX ||
        (uint64_t)ref + (pool[ref - 1u] + 3u) / 4u > pool_dwords)
      return -1;
  }
  for (int64_t i = 0; i < nq; ++i)
    if (q[i].off > qbytes_len || q[i].len > qbytes_len - q[i].off) return -1;
  jgset::Slot* ds = nullptr;
  uint32_t* dp = nullptr;
  uint8_t *dq = nullptr, *dh = nullptr;
  jg_sarg* dsp = nullptr;
  int rc = -2;
  do {
    if (hipMalloc(&ds, sizeof(jgset::Slot) * nslots) != hipSuccess) break;
    if (hipMalloc(&dp, 4 * (size_t)pool_dwords + 16) != hipSuccess) break;
    if (hipMalloc(&dq, qbytes_len + 16) != hipSuccess) break;
    if (hipMalloc(&dsp, sizeof(jg_sarg) * nq) != hipSuccess) break;
    if (hipMalloc(&dh, nq) != hipSuccess) break;
    if (hipMemcpy(ds, slots, sizeof(jgset::Slot) * nslots, hipMemcpyHostToDevice) != hipSuccess) break;
    if (pool_dwords && hipMemcpy(dp, pool, 4 * (size_t)pool_dwords, hipMemcpyHostToDevice) != hipSuccess) break;
    if (qbytes_len && hipMemcpy(dq, qbytes, qbytes_len, hipMemcpyHostToDevice) != hipSuccess) break;
    if (hipMemcpy(dsp, q, sizeof(jg_sarg) * nq, hipMemcpyHostToDevice) != hipSuccess) break;
    if (hipMemset(dh, 0xA5, nq) != hipSuccess) break;
    const jgset::View t{ds, dp, nslots - 1u, maxprobe, seed, n};
    hipLaunchKernelGGL(k_tk_set_probe, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, nullptr, t, dq, dsp, nq, dh);
    if (hipGetLastError() != hipSuccess) break;
    if (hipDeviceSynchronize() != hipSuccess) break;
    if (hipMemcpy(hit_out, dh, nq, hipMemcpyDeviceToHost) != hipSuccess) break;
    rc = 0;
  } while (false);
  (void)hipFree(ds);
  (void)hipFree(dp);
  (void)hipFree(dq);
  (void)hipFree(dsp);
  (void)hipFree(dh);
  return rc;
}
