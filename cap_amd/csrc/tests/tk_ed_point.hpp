// tk_ed_point.hpp -- TEST INFRASTRUCTURE, included at the end of tk_ed.hip (the
// one translation unit of libcapjwt_tk.so that holds kernels/ed25519.hip): the
// production point kernels k_ed_point<WA>, k_ed_point_pf<WA> and
// k_ed_point_split<WA, ED_SPLIT> on SPARSE comb tables, for
// tests/test_gpu_ed_point_exact.py.
//
// The kernels index their tables with compile-time geometry, so the base
// table and each key's table are allocated at full size; they are filled with
// the poison word 0xA5A5A5A5 and only the entries the caller supplies are
// written.  A kernel that reads any entry but the ones its digits name
// computes on poison limbs, and the caller's exact compare fails.
#pragma once

namespace {

constexpr int TKEDP_MAX_KEYS = 2;
constexpr int TKEDP_XYZ_ROWS = 3 * L;            // X, Y, Z (the point kernels leave the prefix rows alone)
static_assert(L == fe::L && L == ED_L, "the xyz rows hold one radix-2^25.5 limb each");

// entry e (ED_STRIDE words at ent + e * ED_STRIDE) -> entry idx[e] of tab0, or
// of tab1 where key[e] == 1; one thread per word.  The host has checked every
// index against its table.
__global__ void k_tk_ed_scatter(uint32_t* tab0, uint32_t* tab1, const int64_t* key, const int64_t* idx,
                                const uint32_t* ent, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * ED_STRIDE) return;
  const int64_t e = i / ED_STRIDE;
  uint32_t* tab = (key && key[e] == 1) ? tab1 : tab0;
  tab[idx[e] * ED_STRIDE + i % ED_STRIDE] = ent[i];
}

}  // namespace

// lanes per token of form 2 (kernels/point_form.hpp ED_SPLIT): the caller's model must split alike
extern "C" int tk_ed_point_split_lanes() { return ED_SPLIT; }

// One call runs the three point kernels of key-table width wa on the same
// tokens: form 0 k_ed_point<wa>, form 1 k_ed_point_pf<wa>, form 2
// k_ed_point_split<wa, ED_SPLIT>, each over [begin, end) of npad padded slots
// (all three multiples of 64) with launch_ed's grid and block.
//   jobs      npad records; only meta is read (a padding lane carries JOB_PAD)
//   status_in npad bytes; every form starts from it
//   siglen    npad decoded signature lengths
//   srows     8 rows x npad: sig[32..64) as little-endian words (the R rows of
//             the device's sigw hold poison: the point kernels do not read R)
//   dig       16 rows x npad: SHA-512(R || A || M) as big-endian words
//   nkeys     1 or 2; key_valid[k] is DevKey::valid of key k (an invalid key
//             still has a table: the kernels load entries before they look)
//   b_idx/b_ent  nb entries of the base table: entry index w * NE + (d - 1)
//                and its ED_STRIDE words
//   a_key/a_idx/a_ent  na entries of the key tables, a_key[e] the key
// Out: xyz_out (3 forms x 30 rows x npad: X, Y, Z limbs, 0xA5A5A5A5 wherever
// the kernel did not write), status_out (3 x npad).
// Refused with -1, nothing allocated or launched, the outputs untouched: wa not
// in ED_WA; npad, begin, end not multiples of 64 or out of order; nkeys not 1
// or 2; an entry index outside its table or an a_key outside the keys; a live
// job of [begin, end) whose key is not below nkeys; live jobs of one 64-slot
// group naming different keys (the one-lane kernels take the wave's key with
// readfirstlane).  Returns 0, or -2 on a HIP error.
extern "C" int tk_ed_point(int wa, int64_t npad, int64_t begin, int64_t end, const JobDev* jobs,
                           const uint8_t* status_in, const uint16_t* siglen, const uint32_t* srows,
                           const uint32_t* dig, int nkeys, const uint8_t* key_valid, const int64_t* b_idx,
                           const uint32_t* b_ent, int64_t nb, const int64_t* a_key, const int64_t* a_idx,
                           const uint32_t* a_ent, int64_t na, uint32_t* xyz_out, uint8_t* status_out) {
  bool tier = false;
  for (int w : ED_WA) tier = tier || w == wa;
  if (!tier) return -1;
  if (npad <= 0 || npad % WAVE != 0 || npad > TKED_MAX_JOBS) return -1;
  if (begin < 0 || begin % WAVE != 0 || end % WAVE != 0 || begin >= end || end > npad) return -1;
  if (nkeys < 1 || nkeys > TKEDP_MAX_KEYS || nb < 0 || na < 0 || nb > TKED_MAX_JOBS || na > TKED_MAX_JOBS) return -1;
  if (!jobs || !status_in || !siglen || !srows || !dig || !key_valid || !xyz_out || !status_out) return -1;
  if ((nb && (!b_idx || !b_ent)) || (na && (!a_key || !a_idx || !a_ent))) return -1;
  const int64_t b_entries = (int64_t)ed_windows(true) * ed_entries(true);
  const int64_t a_entries = (int64_t)ed_windows_w(wa) * ((int64_t)1 << (wa - 1));
  for (int64_t e = 0; e < nb; ++e)
    if (b_idx[e] < 0 || b_idx[e] >= b_entries) return -1;
  for (int64_t e = 0; e < na; ++e)
    if (a_key[e] < 0 || a_key[e] >= nkeys || a_idx[e] < 0 || a_idx[e] >= a_entries) return -1;
  for (int64_t g = begin; g < end; g += WAVE) {
    int key = -1;
    for (int64_t p = g; p < g + WAVE; ++p) {
      if (!job_live(jobs[p])) continue;
      if (job_key(jobs[p]) >= nkeys) return -1;
      if (key >= 0 && job_key(jobs[p]) != key) return -1;
      key = job_key(jobs[p]);
    }
  }

  const size_t np = (size_t)npad;
  const size_t b_bytes = (size_t)ed_table_words(true) * 4, a_bytes = (size_t)ed_table_words_w(wa) * 4;
  const size_t xyz_bytes = (size_t)TKEDP_XYZ_ROWS * np * 4;
  JobDev* d_jobs = (JobDev*)tked_alloc(np * sizeof(JobDev));
  uint8_t* d_status = (uint8_t*)tked_alloc(np);
  uint16_t* d_siglen = (uint16_t*)tked_alloc(np * 2);
  uint32_t* d_sigw = (uint32_t*)tked_alloc((size_t)16 * np * 4);
  uint32_t* d_dig = (uint32_t*)tked_alloc((size_t)16 * np * 4);
  uint32_t* d_xyz = (uint32_t*)tked_alloc(xyz_bytes);
  DevKey* d_keys = (DevKey*)tked_alloc(TKEDP_MAX_KEYS * sizeof(DevKey));
  int64_t* d_bidx = (int64_t*)tked_alloc((size_t)nb * 8);
  uint32_t* d_bent = (uint32_t*)tked_alloc((size_t)nb * ED_STRIDE * 4);
  int64_t* d_akey = (int64_t*)tked_alloc((size_t)na * 8);
  int64_t* d_aidx = (int64_t*)tked_alloc((size_t)na * 8);
  uint32_t* d_aent = (uint32_t*)tked_alloc((size_t)na * ED_STRIDE * 4);
  uint32_t* d_btab = (uint32_t*)tked_alloc(b_bytes);
  uint32_t* d_atab[TKEDP_MAX_KEYS] = {nullptr, nullptr};
  bool ok = d_jobs && d_status && d_siglen && d_sigw && d_dig && d_xyz && d_keys && d_bidx && d_bent && d_akey &&
            d_aidx && d_aent && d_btab;
  for (int k = 0; k < nkeys; ++k) {
    d_atab[k] = (uint32_t*)tked_alloc(a_bytes);
    ok = ok && d_atab[k];
  }
  auto chk = [&](hipError_t e) { ok = ok && e == hipSuccess; };
  if (ok) {
    DevKey hk[TKEDP_MAX_KEYS] = {};
    for (int k = 0; k < nkeys; ++k) {
      hk[k].cls = PF_CLS_ED25519;
      hk[k].valid = key_valid[k] ? 1 : 0;
      hk[k].kbytes = 32;
      hk[k].tab = (uint64_t)(uintptr_t)d_atab[k];
      hk[k].tab_w = wa;
    }
    chk(hipMemcpy(d_keys, hk, sizeof(hk), hipMemcpyHostToDevice));
    chk(hipMemcpy(d_jobs, jobs, np * sizeof(JobDev), hipMemcpyHostToDevice));
    chk(hipMemcpy(d_siglen, siglen, np * 2, hipMemcpyHostToDevice));
    chk(hipMemset(d_sigw, 0xA5, (size_t)16 * np * 4));      // (the R rows: the point kernels read S alone)
    chk(hipMemcpy(d_sigw + (size_t)8 * np, srows, (size_t)8 * np * 4, hipMemcpyHostToDevice));
    chk(hipMemcpy(d_dig, dig, (size_t)16 * np * 4, hipMemcpyHostToDevice));
    chk(hipMemset(d_btab, 0xA5, b_bytes));
    for (int k = 0; k < nkeys; ++k) chk(hipMemset(d_atab[k], 0xA5, a_bytes));
    if (nb) {
      chk(hipMemcpy(d_bidx, b_idx, (size_t)nb * 8, hipMemcpyHostToDevice));
      chk(hipMemcpy(d_bent, b_ent, (size_t)nb * ED_STRIDE * 4, hipMemcpyHostToDevice));
    }
    if (na) {
      chk(hipMemcpy(d_akey, a_key, (size_t)na * 8, hipMemcpyHostToDevice));
      chk(hipMemcpy(d_aidx, a_idx, (size_t)na * 8, hipMemcpyHostToDevice));
      chk(hipMemcpy(d_aent, a_ent, (size_t)na * ED_STRIDE * 4, hipMemcpyHostToDevice));
    }
    chk(hipDeviceSynchronize());
  }
  if (ok && nb) {
    hipLaunchKernelGGL(k_tk_ed_scatter, dim3((unsigned)((nb * ED_STRIDE + 255) / 256)), dim3(256), 0, 0, d_btab,
                       (uint32_t*)nullptr, (const int64_t*)nullptr, d_bidx, d_bent, nb);
    chk(hipGetLastError());
  }
  if (ok && na) {
    hipLaunchKernelGGL(k_tk_ed_scatter, dim3((unsigned)((na * ED_STRIDE + 255) / 256)), dim3(256), 0, 0, d_atab[0],
                       d_atab[1], d_akey, d_aidx, d_aent, na);
    chk(hipGetLastError());
  }
  if (ok) chk(hipDeviceSynchronize());
  for (int form = 0; form < 3 && ok; ++form) {
    chk(hipMemcpy(d_status, status_in, np, hipMemcpyHostToDevice));
    chk(hipMemset(d_xyz, 0xA5, xyz_bytes));
    chk(hipDeviceSynchronize());
    if (!ok) break;
    EdArgs ea{};
    ea.jobs = d_jobs; ea.keys = d_keys; ea.keyblob = nullptr;
    ea.sigw = d_sigw; ea.dig = d_dig; ea.status = d_status; ea.siglen = d_siglen;
    ea.verdict_pad = nullptr;
    ea.xyz = d_xyz;
    ea.btab = d_btab;
    ea.npad = npad; ea.begin = begin; ea.end = end; ea.wa = wa;
    const int lanes = form == 2 ? ED_SPLIT : 1;
    const dim3 g((unsigned)((end - begin) * lanes / WAVE)), b(WAVE);     // launch_ed's shape
    with_wa(wa, [&](auto w) {
      constexpr int WA = decltype(w)::value;
      if (form == 0) hipLaunchKernelGGL(k_ed_point<WA>, g, b, 0, 0, ea);
      else if (form == 1) hipLaunchKernelGGL(k_ed_point_pf<WA>, g, b, 0, 0, ea);
      else hipLaunchKernelGGL((k_ed_point_split<WA, ED_SPLIT>), g, b, 0, 0, ea);
    });
    chk(hipGetLastError());
    chk(hipDeviceSynchronize());
    if (!ok) break;
    chk(hipMemcpy(xyz_out + (size_t)form * TKEDP_XYZ_ROWS * np, d_xyz, xyz_bytes, hipMemcpyDeviceToHost));
    chk(hipMemcpy(status_out + (size_t)form * np, d_status, np, hipMemcpyDeviceToHost));
  }
  for (void* ptr : {(void*)d_jobs, (void*)d_status, (void*)d_siglen, (void*)d_sigw, (void*)d_dig, (void*)d_xyz,
                    (void*)d_keys, (void*)d_bidx, (void*)d_bent, (void*)d_akey, (void*)d_aidx, (void*)d_aent,
                    (void*)d_btab, (void*)d_atab[0], (void*)d_atab[1]})
    if (ptr) (void)hipFree(ptr);
  return ok ? 0 : -2;
}
