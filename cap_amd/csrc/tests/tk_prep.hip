// tk_prep.hip -- TEST INFRASTRUCTURE (libcapjwt_tk.so only, never the product
// path): the prep stage alone (kernels/prep.hip k_prep_mid + k_prep through the
// production launch_prep), so tests/test_gpu_prep_exact.py can compare every
// digest word, every decoded signature row, the status byte and the decoded
// length of every padded slot with hashlib / base64 -- the verify chain only
// tells accept from reject.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../kernels/ecdsa.hpp"
#include "../kernels/rsa.hpp"
#include "../kernels/prep.hip"   // kernels in an anonymous namespace: this TU's own copy

namespace {

constexpr uint64_t TKP_ARENA_SLACK = 256;       // jg_runtime.cpp ARENA_SLACK
constexpr int64_t TKP_MAX_JOBS = 1 << 20;
constexpr int TKP_MAX_KEYS = 4096;

// rows of the decoded signature the class's arithmetic kernel reads
// (jg_runtime.cpp cls_rows_sig); l4 = the largest RSA-4K+ layout among the keys
int tkp_rows_sig(int c, int l4) {
  switch (c) {
    case CLS_RSA2K: case CLS_RSA3K: return rsa_sig_rows(c);
    case CLS_RSA4K: return rsa_sig_rows_l(l4);
    case CLS_P256: case CLS_P384: case CLS_P521: return EC_S_ROW + 17;
    case CLS_ED25519: return 16;
    default: return 0;
  }
}

bool tkp_limbs_ok(int cls, uint32_t nl) {
  if (cls == CLS_RSA2K || cls == CLS_RSA3K) return nl == (uint32_t)rsa_limbs(cls);
  for (int i = 0; i < RSA4K_NLAYOUT; ++i)
    if (nl == (uint32_t)rsa4k_layout_limbs(i)) return true;
  return false;
}

void* tkp_alloc(size_t bytes) {
  void* d = nullptr;
  return hipMalloc(&d, bytes ? bytes : 16) == hipSuccess ? d : nullptr;
}

}  // namespace

// cls: CLS_RSA2K .. CLS_ED25519.  hash_mask: bit 0 = SHA-256 algs present, bit
// 1 = SHA-384/512 (the variant launch_prep picks; the caller keeps the algs of
// the jobs inside it).  use_mid != 0: the shared-block-0 scratch is supplied,
// sized as the runtime sizes it.  arena: arena_len bytes; the device copy gets
// 256 zeroed bytes of slack behind it.  jobs: njobs records in padded order --
// njobs a multiple of 64, every wave on one key, padding lanes carry JOB_PAD
// and zero offsets.  Per key: nlimbs[key] (RSA classes) and 32 public-key
// bytes at pub + 32 key (Ed25519, placed at the key's aux_off).
// Out, for every padded slot: dig (DIG_ROWS x njobs), sigw (SIGW_ROWS x njobs),
// status (njobs), siglen (njobs); dig and sigw hold 0xA5A5A5A5 wherever the
// kernels did not write.  *zrows_out / *ec_words_out: the values launched with.
// mid_out (may be null; PREP_MID_WORDS x nkeys words): the shared-block-0 slots
// after the launch when use_mid != 0 -- still 0xA5A5A5A5 for a key whose run
// recorded nothing, or when launch_prep dropped the midstate pass.
// Returns 0; -1 on a bad argument (nothing is launched); -2 on a HIP error.
extern "C" int tk_prep(int cls, int hash_mask, int use_mid, const uint8_t* arena, uint64_t arena_len,
                       const JobDev* jobs, int64_t njobs, int nkeys, const uint32_t* nlimbs, const uint8_t* pub,
                       uint32_t* dig, uint32_t* sigw, uint8_t* status, uint16_t* siglen, int* zrows_out,
                       int* ec_words_out, uint32_t* mid_out) {
  if (cls < CLS_RSA2K || cls > CLS_ED25519 || hash_mask < 1 || hash_mask > 3) return -1;
  if (!arena || !jobs || !dig || !sigw || !status || !siglen) return -1;
  if (arena_len == 0 || arena_len + TKP_ARENA_SLACK >= (uint64_t(1) << 32)) return -1;
  if (njobs <= 0 || njobs % WAVE != 0 || njobs > TKP_MAX_JOBS) return -1;
  if (nkeys <= 0 || nkeys > TKP_MAX_KEYS) return -1;
  const bool rsa = cls <= CLS_RSA4K, ed = cls == CLS_ED25519;
  if ((rsa && !nlimbs) || (ed && !pub)) return -1;
  int l4 = 0;
  if (rsa)
    for (int k = 0; k < nkeys; ++k) {
      if (!tkp_limbs_ok(cls, nlimbs[k])) return -1;
      l4 = std::max(l4, (int)nlimbs[k]);
    }
  const int zrows = tkp_rows_sig(cls, l4);
  const int ec_words = (cls >= CLS_P256 && cls <= CLS_P521) ? ec_sig_words(cls) : 0;
  if (zrows <= 0 || zrows > SIGW_ROWS) return -1;
  for (int64_t w = 0; w < njobs; w += WAVE) {
    const int key = job_key(jobs[w]);
    if (key >= nkeys) return -1;
    for (int64_t p = w; p < w + WAVE; ++p) {
      const JobDev& j = jobs[p];
      if (job_key(j) != key) return -1;                       // the key is wave-uniform
      if (!job_live(j)) {
        if (j.off || j.sig_in_len || j.sig_off || job_siglen(j)) return -1;
        continue;
      }
      const int alg = job_alg(j);
      if (alg < 1 || alg > 10) return -1;
      const int hbit = (alg == 1 || alg == 4 || alg == 7) ? 1 : 2;
      if (!ed && !(hash_mask & hbit)) return -1;               // the variant launched has this alg's SHA
      if ((uint64_t)j.off + j.sig_in_len > arena_len) return -1;
      if ((uint64_t)j.sig_off + job_siglen(j) > arena_len) return -1;
      if (job_siglen(j) >= JOB_SIGLEN_MAX) return -1;
    }
  }

  const size_t np = (size_t)njobs;
  std::vector<DevKey> keys((size_t)nkeys);
  std::vector<uint32_t> blob((size_t)nkeys * 8 + 8, 0);
  for (int k = 0; k < nkeys; ++k) {
    DevKey K{};
    K.kind = rsa ? 1 : ed ? 3 : 2;
    K.cls = cls;
    K.valid = 1;
    K.nlimbs = rsa ? nlimbs[k] : 0u;
    K.aux_off = (uint64_t)k * 8;
    if (ed) std::memcpy(&blob[(size_t)k * 8], pub + (size_t)k * 32, 32);
    keys[(size_t)k] = K;
  }

  const size_t mid_bytes = sizeof(uint32_t) * PREP_MID_WORDS * (size_t)std::max(nkeys, 1);
  uint8_t* d_arena = (uint8_t*)tkp_alloc(arena_len + TKP_ARENA_SLACK);
  JobDev* d_jobs = (JobDev*)tkp_alloc(np * sizeof(JobDev));
  DevKey* d_keys = (DevKey*)tkp_alloc(keys.size() * sizeof(DevKey));
  uint32_t* d_blob = (uint32_t*)tkp_alloc(blob.size() * sizeof(uint32_t));
  uint32_t* d_sigw = (uint32_t*)tkp_alloc((size_t)SIGW_ROWS * np * sizeof(uint32_t));
  uint32_t* d_dig = (uint32_t*)tkp_alloc((size_t)DIG_ROWS * np * sizeof(uint32_t));
  uint8_t* d_status = (uint8_t*)tkp_alloc(np);
  uint16_t* d_siglen = (uint16_t*)tkp_alloc(np * sizeof(uint16_t));
  uint32_t* d_mid = use_mid ? (uint32_t*)tkp_alloc(mid_bytes) : nullptr;
  bool ok = d_arena && d_jobs && d_keys && d_blob && d_sigw && d_dig && d_status && d_siglen && (!use_mid || d_mid);
  auto chk = [&](hipError_t e) { ok = ok && e == hipSuccess; };
  if (ok) {
    chk(hipMemcpy(d_arena, arena, arena_len, hipMemcpyHostToDevice));
    chk(hipMemset(d_arena + arena_len, 0, TKP_ARENA_SLACK));
    chk(hipMemcpy(d_jobs, jobs, np * sizeof(JobDev), hipMemcpyHostToDevice));
    chk(hipMemcpy(d_keys, keys.data(), keys.size() * sizeof(DevKey), hipMemcpyHostToDevice));
    chk(hipMemcpy(d_blob, blob.data(), blob.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    // poison: rows the kernels leave unwritten read back as 0xA5A5A5A5
    chk(hipMemset(d_sigw, 0xA5, (size_t)SIGW_ROWS * np * sizeof(uint32_t)));
    chk(hipMemset(d_dig, 0xA5, (size_t)DIG_ROWS * np * sizeof(uint32_t)));
    chk(hipMemset(d_status, 0xA5, np));
    chk(hipMemset(d_siglen, 0xA5, np * sizeof(uint16_t)));
    if (d_mid) chk(hipMemset(d_mid, 0xA5, mid_bytes));
    chk(hipDeviceSynchronize());
  }
  if (ok) {
    PrepArgs pa{};
    pa.arena = d_arena; pa.jobs = d_jobs; pa.keys = d_keys; pa.keyblob = d_blob;
    pa.sigw = d_sigw; pa.dig = d_dig; pa.status = d_status; pa.siglen = d_siglen;
    pa.npad = njobs; pa.begin = 0; pa.end = njobs;
    pa.zrows = zrows; pa.ec_words = ec_words;
    pa.mid = d_mid;
    launch_prep(cls, hash_mask, pa, 0);
    chk(hipGetLastError());
    chk(hipDeviceSynchronize());
  }
  if (ok) {
    chk(hipMemcpy(sigw, d_sigw, (size_t)SIGW_ROWS * np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    chk(hipMemcpy(dig, d_dig, (size_t)DIG_ROWS * np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    chk(hipMemcpy(status, d_status, np, hipMemcpyDeviceToHost));
    chk(hipMemcpy(siglen, d_siglen, np * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (d_mid && mid_out) chk(hipMemcpy(mid_out, d_mid, mid_bytes, hipMemcpyDeviceToHost));
  }
  for (void* ptr : {(void*)d_arena, (void*)d_jobs, (void*)d_keys, (void*)d_blob, (void*)d_sigw, (void*)d_dig,
                    (void*)d_status, (void*)d_siglen, (void*)d_mid})
    if (ptr) (void)hipFree(ptr);
  if (zrows_out) *zrows_out = zrows;
  if (ec_words_out) *ec_words_out = ec_words;
  return ok ? 0 : -2;
}
