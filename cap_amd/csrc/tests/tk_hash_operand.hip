// tk_hash_operand.hip -- TEST INFRASTRUCTURE (libcapjwt_tk.so only, never the
// product path): the hash-operand kernel alone (kernels/hash_operand.hip
// k_hash_operand through the production launch_hash_operand), so
// tests/test_gpu_hash_operand.py can compare every operand byte and every span
// it writes with hashlib + base64 -- the scan behind it only tells equal from
// not equal.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../kernels/hash_operand.hip"   // the kernel is in an anonymous namespace: this TU's own copy

namespace {
constexpr uint64_t TKH_SLACK = 256;      // jg_runtime.cpp ARENA_SLACK
}

// bytes: bytes_len source bytes; the device copy gets 256 zeroed bytes of slack
// behind it.  src: njobs x nhash records.  The operand buffer is op_base + 44 *
// njobs * nhash bytes and the span table njobs x (nstr + nhash) records, both
// filled with 0xA5 before the launch and copied out whole: op_out, spans_out.
// Returns 0; -1 for arguments the runtime would have refused (the kernel is not
// launched); -2 on a HIP error.
extern "C" int tk_hash_operand(const uint8_t* bytes, uint64_t bytes_len, const jg_hsrc* src, int64_t njobs,
                               uint32_t nhash, uint32_t nstr, uint32_t op_base, uint8_t* op_out, jg_sarg* spans_out) {
  if (njobs <= 0 || njobs > (1 << 20) || nhash == 0 || nhash > JG_MAX_HASH_ARGS || nstr + nhash > JG_MAX_ARGS ||
      (op_base & 3u) || op_base > (1u << 20) || bytes_len >= (uint64_t(1) << 31) || !src || !op_out || !spans_out ||
      (bytes_len && !bytes))
    return -1;
  const int64_t n = njobs * nhash;
  for (int64_t t = 0; t < n; ++t)
    if (src[t].fam > JG_SHA512 || src[t].len > JG_HASH_SRC_MAX || src[t].off > bytes_len ||
        src[t].len > bytes_len - src[t].off)
      return -1;
  const size_t op_len = op_base + (size_t)n * jghop::kSlot, sp_len = sizeof(jg_sarg) * njobs * (nstr + nhash);
  uint8_t *db = nullptr, *dop = nullptr;
  jg_hsrc* ds = nullptr;
  jg_sarg* dsp = nullptr;
  int rc = -2;
  do {
    if (hipMalloc(&db, bytes_len + TKH_SLACK) != hipSuccess) break;
    if (hipMalloc(&ds, sizeof(jg_hsrc) * n) != hipSuccess) break;
    if (hipMalloc(&dop, op_len + TKH_SLACK) != hipSuccess) break;
    if (hipMalloc(&dsp, sp_len) != hipSuccess) break;
    if (hipMemset(db + bytes_len, 0, TKH_SLACK) != hipSuccess) break;
    if (bytes_len && hipMemcpy(db, bytes, bytes_len, hipMemcpyHostToDevice) != hipSuccess) break;
    if (hipMemcpy(ds, src, sizeof(jg_hsrc) * n, hipMemcpyHostToDevice) != hipSuccess) break;
    if (hipMemset(dop, 0xA5, op_len + TKH_SLACK) != hipSuccess) break;
    if (hipMemset(dsp, 0xA5, sp_len) != hipSuccess) break;
    launch_hash_operand(db, ds, njobs, nhash, nstr, op_base, dop, dsp, nullptr);
    if (hipGetLastError() != hipSuccess) break;
    if (hipDeviceSynchronize() != hipSuccess) break;
    if (hipMemcpy(op_out, dop, op_len, hipMemcpyDeviceToHost) != hipSuccess) break;
    if (hipMemcpy(spans_out, dsp, sp_len, hipMemcpyDeviceToHost) != hipSuccess) break;
    rc = 0;
  } while (false);
  (void)hipFree(db);
  (void)hipFree(ds);
  (void)hipFree(dop);
  (void)hipFree(dsp);
  return rc;
}
