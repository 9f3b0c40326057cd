// tk_ed.hip -- TEST INFRASTRUCTURE (libcapjwt_tk.so only, never the product
// path): the stages of kernels/ed25519.hip alone, for
// tests/test_gpu_ed_exact.py and tests/test_gpu_ed_point_exact.py:
//   tk_ed_scalar : k = H mod L (ed_k_mod_l), the S check (ed_s_ok) and the
//                  signed recoding (recode) of k at every key-table tier and
//                  of S at the base-point width, per lane;
//   tk_ed_finish : the production k_ed_finish at any tokens-per-thread B --
//                  production picks B > 1 only from 262,144 padded tokens up;
//   tk_ed_point  : the production k_ed_point, k_ed_point_pf and
//                  k_ed_point_split on sparse comb tables (tk_ed_point.hpp;
//                  it lives in this translation unit because ed25519.hip
//                  defines launch_ed and its kin, which one library holds once).
// The verify chain only tells accept from reject, on SHA-random k.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

#include "../kernels/ed25519.hip"   // kernels in an anonymous namespace: this TU's own copy

namespace {

constexpr int64_t TKED_MAX_JOBS = 1 << 20;
constexpr int TKED_NB = ed_windows(true);
constexpr int TKED_KROWS = ed_windows_w(24) + ed_windows_w(22) + ed_windows_w(20) + ed_windows_w(18) + ed_windows_w(16);
constexpr int TKED_XYZ_ROWS = 4 * L;             // X, Y, Z, then k_ed_finish's prefix products

__global__ void k_tk_ed_scalar(const uint32_t* dig, const uint32_t* srows, int n, uint32_t* kout, uint8_t* sok,
                               int* kdig, int* sdig) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t hw[16], k[L], sw[8], s[L];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const uint32_t x = dig[(int64_t)q * n + i];     // big-endian digest words, as the point kernels read them
    hw[q] = (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
  }
  ed_k_mod_l(k, hw);
#pragma unroll
  for (int j = 0; j < L; ++j) kout[(int64_t)j * n + i] = k[j];
#pragma unroll
  for (int q = 0; q < 8; ++q) sw[q] = srows[(int64_t)q * n + i];
  sok[i] = ed_s_ok(s, sw) ? 1 : 0;
  recode<ed_comb_w(true), TKED_NB>(sdig + i, s, n);
  int* kd = kdig + i;
  recode<24, ed_windows_w(24)>(kd, k, n); kd += (int64_t)ed_windows_w(24) * n;
  recode<22, ed_windows_w(22)>(kd, k, n); kd += (int64_t)ed_windows_w(22) * n;
  recode<20, ed_windows_w(20)>(kd, k, n); kd += (int64_t)ed_windows_w(20) * n;
  recode<18, ed_windows_w(18)>(kd, k, n); kd += (int64_t)ed_windows_w(18) * n;
  recode<16, ed_windows_w(16)>(kd, k, n);
}

void* tked_alloc(size_t bytes) {
  void* d = nullptr;
  return hipMalloc(&d, bytes ? bytes : 16) == hipSuccess ? d : nullptr;
}

}  // namespace

// n lanes (1 .. 65536).  dig: 16 rows x n, SHA-512 digest as big-endian words
// (row q = digest bytes 4q .. 4q+3); srows: 8 rows x n, sig[32..64) as
// little-endian words.  Out, all poisoned with 0xA5 before the launch:
// k (10 rows x n, 28-bit limbs of H mod L), s_ok (n), kdig (the windows of k at
// W = 24, 22, 20, 18, 16 in that order, ed_windows_w(W) rows x n each), sdig
// (ed_windows(true) rows x n: S at the base-point width).
// Returns 0; -1 on a bad argument (nothing is launched); -2 on a HIP error.
extern "C" int tk_ed_scalar(int n, const uint32_t* dig, const uint32_t* srows, uint32_t* k, uint8_t* s_ok,
                            int32_t* kdig, int32_t* sdig) {
  static_assert(ED_WA[0] == 24 && ED_WA[1] == 22 && ED_WA[2] == 20 && ED_WA[3] == 18 && ED_WA[4] == 16, "tiers");
  if (n <= 0 || n > 65536 || !dig || !srows || !k || !s_ok || !kdig || !sdig) return -1;
  const size_t N = (size_t)n;
  uint32_t* d_dig = (uint32_t*)tked_alloc(16 * N * 4);
  uint32_t* d_s = (uint32_t*)tked_alloc(8 * N * 4);
  uint32_t* d_k = (uint32_t*)tked_alloc(L * N * 4);
  uint8_t* d_ok = (uint8_t*)tked_alloc(N);
  int* d_kd = (int*)tked_alloc(TKED_KROWS * N * 4);
  int* d_sd = (int*)tked_alloc(TKED_NB * N * 4);
  bool ok = d_dig && d_s && d_k && d_ok && d_kd && d_sd;
  auto chk = [&](hipError_t e) { ok = ok && e == hipSuccess; };
  if (ok) {
    chk(hipMemcpy(d_dig, dig, 16 * N * 4, hipMemcpyHostToDevice));
    chk(hipMemcpy(d_s, srows, 8 * N * 4, hipMemcpyHostToDevice));
    chk(hipMemset(d_k, 0xA5, L * N * 4));
    chk(hipMemset(d_ok, 0xA5, N));
    chk(hipMemset(d_kd, 0xA5, TKED_KROWS * N * 4));
    chk(hipMemset(d_sd, 0xA5, TKED_NB * N * 4));
    chk(hipDeviceSynchronize());
  }
  if (ok) {
    hipLaunchKernelGGL(k_tk_ed_scalar, dim3((unsigned)((n + WAVE - 1) / WAVE)), dim3(WAVE), 0, 0, d_dig, d_s, n, d_k, d_ok,
                       d_kd, d_sd);
    chk(hipGetLastError());
    chk(hipDeviceSynchronize());
  }
  if (ok) {
    chk(hipMemcpy(k, d_k, L * N * 4, hipMemcpyDeviceToHost));
    chk(hipMemcpy(s_ok, d_ok, N, hipMemcpyDeviceToHost));
    chk(hipMemcpy(kdig, d_kd, TKED_KROWS * N * 4, hipMemcpyDeviceToHost));
    chk(hipMemcpy(sdig, d_sd, TKED_NB * N * 4, hipMemcpyDeviceToHost));
  }
  for (void* ptr : {(void*)d_dig, (void*)d_s, (void*)d_k, (void*)d_ok, (void*)d_kd, (void*)d_sd})
    if (ptr) (void)hipFree(ptr);
  return ok ? 0 : -2;
}

// The launch shape launch_ed picks for a finish stage of n padded tokens
// (kernels/inv_shape.hpp).  Returns 0; -1 on a bad argument.
extern "C" int tk_ed_finish_shape(int64_t n, int* B, int64_t* S, int* wpb, unsigned* grid) {
  if (n <= 0 || n % WAVE != 0 || !B || !S || !wpb || !grid) return -1;
  const InvShape sh = inv_shape(n, ED_FINISH_WPB, 0);
  *B = sh.B; *S = sh.S; *wpb = sh.wpb; *grid = sh.grid;
  return 0;
}

// B: tokens per thread, 1..16.  The launch covers [begin, end) of npad padded
// slots, all three multiples of 64, with launch_ed's grid and block.  jobs:
// npad records (only meta is read: a padding lane carries JOB_PAD); status_in:
// npad bytes; xyz_in: 30 rows x npad, X, Y, Z of R' in radix 2^25.5 -- every
// limb of a live ST_OK slot of [begin, end) below 2^31 (what fe_to_mont
// accepts; other slots are not read); rrows: 8 rows x npad, sig[0..32) as
// little-endian words.
// Out: verdict (npad, 0xA5 wherever the kernel did not write), xyz_out (40 rows
// x npad: X, Y, Z as the kernel left them, then the prefix-product rows,
// 0xA5A5A5A5 wherever unwritten), status_out (npad).
// Returns 0; -1 on a bad argument (nothing is launched); -2 on a HIP error.
extern "C" int tk_ed_finish(int B, int64_t npad, int64_t begin, int64_t end, const JobDev* jobs,
                            const uint8_t* status_in, const uint32_t* xyz_in, const uint32_t* rrows, uint8_t* verdict,
                            uint32_t* xyz_out, uint8_t* status_out) {
  if (B < 1 || B > 16) return -1;
  if (npad <= 0 || npad % WAVE != 0 || npad > TKED_MAX_JOBS) return -1;
  if (begin < 0 || begin % WAVE != 0 || end % WAVE != 0 || begin >= end || end > npad) return -1;
  if (!jobs || !status_in || !xyz_in || !rrows || !verdict || !xyz_out || !status_out) return -1;
  const size_t np = (size_t)npad;
  for (int64_t p = begin; p < end; ++p) {
    if (!job_live(jobs[p]) || status_in[p] != ST_OK) continue;
    for (int r = 0; r < 3 * L; ++r)
      if (xyz_in[(size_t)r * np + (size_t)p] >> 31) return -1;
  }

  JobDev* d_jobs = (JobDev*)tked_alloc(np * sizeof(JobDev));
  uint8_t* d_status = (uint8_t*)tked_alloc(np);
  uint32_t* d_xyz = (uint32_t*)tked_alloc((size_t)TKED_XYZ_ROWS * np * 4);
  uint32_t* d_sigw = (uint32_t*)tked_alloc((size_t)16 * np * 4);
  uint8_t* d_verdict = (uint8_t*)tked_alloc(np);
  bool ok = d_jobs && d_status && d_xyz && d_sigw && d_verdict;
  auto chk = [&](hipError_t e) { ok = ok && e == hipSuccess; };
  if (ok) {
    chk(hipMemcpy(d_jobs, jobs, np * sizeof(JobDev), hipMemcpyHostToDevice));
    chk(hipMemcpy(d_status, status_in, np, hipMemcpyHostToDevice));
    chk(hipMemset(d_xyz, 0xA5, (size_t)TKED_XYZ_ROWS * np * 4));
    chk(hipMemcpy(d_xyz, xyz_in, (size_t)3 * L * np * 4, hipMemcpyHostToDevice));
    chk(hipMemset(d_sigw, 0xA5, (size_t)16 * np * 4));     // (the S rows: k_ed_finish reads R alone)
    chk(hipMemcpy(d_sigw, rrows, (size_t)8 * np * 4, hipMemcpyHostToDevice));
    chk(hipMemset(d_verdict, 0xA5, np));
    chk(hipDeviceSynchronize());
  }
  if (ok) {
    EdArgs ea{};
    ea.jobs = d_jobs; ea.keys = nullptr; ea.keyblob = nullptr;
    ea.sigw = d_sigw; ea.dig = nullptr; ea.status = d_status; ea.siglen = nullptr;
    ea.verdict_pad = d_verdict;
    ea.xyz = d_xyz;
    ea.btab = nullptr;
    ea.npad = npad; ea.begin = begin; ea.end = end; ea.wa = 16;
    const int64_t n = end - begin, S = (n + B - 1) / B;
    constexpr int TPB = WAVE * ED_FINISH_WPB;
    hipLaunchKernelGGL(k_ed_finish, dim3((unsigned)((S + TPB - 1) / TPB)), dim3(TPB), 0, 0, ea, B);
    chk(hipGetLastError());
    chk(hipDeviceSynchronize());
  }
  if (ok) {
    chk(hipMemcpy(verdict, d_verdict, np, hipMemcpyDeviceToHost));
    chk(hipMemcpy(xyz_out, d_xyz, (size_t)TKED_XYZ_ROWS * np * 4, hipMemcpyDeviceToHost));
    chk(hipMemcpy(status_out, d_status, np, hipMemcpyDeviceToHost));
  }
  for (void* ptr : {(void*)d_jobs, (void*)d_status, (void*)d_xyz, (void*)d_sigw, (void*)d_verdict})
    if (ptr) (void)hipFree(ptr);
  return ok ? 0 : -2;
}

#include "tk_ed_point.hpp"
