// tk_ec_scalar.hip -- TEST INFRASTRUCTURE (libcapjwt_tk.so only, never the
// product path): the production k_ec_scalar_batch alone, at any tokens-per-
// thread B, so tests/test_gpu_ec_scalar_exact.py can compare every signed digit
// of u1 and u2, the status byte and the exception counter of every padded slot
// with a big-integer model -- the verify chain only tells accept from reject,
// and production picks B > 1 only from 262,144 padded tokens upward.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <vector>

#include "tk_ec_scalar.hpp"

bool tkes_launch_p256(int wq, int wpb, const EcArgs& a, int B) {
  if (wpb == EC_SCALAR_WPB) {
    if (wq == 26) tkes_launch<CurveP256W<26>, EC_SCALAR_WPB>(a, B);
    else if (wq == 24) tkes_launch<CurveP256W<24>, EC_SCALAR_WPB>(a, B);
    else if (wq == 22) tkes_launch<CurveP256W<22>, EC_SCALAR_WPB>(a, B);
    else if (wq == 20) tkes_launch<CurveP256W<20>, EC_SCALAR_WPB>(a, B);
    else return false;
    return true;
  }
  if (wpb == 1 && wq == 20) {
    tkes_launch<CurveP256W<20>, 1>(a, B);
    return true;
  }
  return false;
}

bool tkes_launch_p384(int wq, int wpb, const EcArgs& a, int B) {
  if (wpb == EC_SCALAR_WPB) {
    if (wq == 24) tkes_launch<CurveP384W<24>, EC_SCALAR_WPB>(a, B);
    else if (wq == 20) tkes_launch<CurveP384W<20>, EC_SCALAR_WPB>(a, B);
    else if (wq == 18) tkes_launch<CurveP384W<18>, EC_SCALAR_WPB>(a, B);
    else if (wq == 16) tkes_launch<CurveP384W<16>, EC_SCALAR_WPB>(a, B);
    else return false;
    return true;
  }
  if (wpb == 1 && wq == 16) {
    tkes_launch<CurveP384W<16>, 1>(a, B);
    return true;
  }
  return false;
}

namespace {

constexpr int64_t TKES_MAX_JOBS = 1 << 20;
constexpr int TKES_MAX_KEYS = 4096;
constexpr int TKES_SIG_ROWS = EC_S_ROW + 17;    // r rows 0.., s rows EC_S_ROW.., the widest alg's 17 words each

bool tkes_width_ok(int cls, int wq, int wpb) {
  if (wpb != 1 && wpb != EC_SCALAR_WPB) return false;
  const int* t = cls == CLS_P256 ? EC_P256_WQ : cls == CLS_P384 ? EC_P384_WQ : EC_P521_WQ;
  const int nt = cls == CLS_P521 ? 3 : 4;
  if (wpb == 1 && EC_SCALAR_WPB != 1) return wq == t[nt - 1];   // WPB = 1: the narrowest width only
  for (int i = 0; i < nt; ++i)
    if (t[i] == wq) return true;
  return false;
}

void* tkes_alloc(size_t bytes) {
  void* d = nullptr;
  return hipMalloc(&d, bytes ? bytes : 16) == hipSuccess ? d : nullptr;
}

}  // namespace

// The launch shape launch_chain picks for a scalar stage of n padded tokens
// (kernels/inv_shape.hpp).  Returns 0; -1 on a bad argument.
extern "C" int tk_ec_scalar_shape(int64_t n, int* B, int64_t* S, int* wpb, unsigned* grid) {
  if (n <= 0 || n % WAVE != 0 || !B || !S || !wpb || !grid) return -1;
  const InvShape sh = inv_shape(n, EC_SCALAR_WPB, EC_SCALAR_SOLO_MAX);
  *B = sh.B; *S = sh.S; *wpb = sh.wpb; *grid = sh.grid;
  return 0;
}

// The point kernel launch_chain (cls = CLS_P256 .. CLS_P521; force: its
// debugging switch) or launch_ed (CLS_ED25519) picks for a width run of n
// padded tokens (kernels/point_form.hpp).  Returns 0; -1 on a bad argument.
extern "C" int tk_point_form(int cls, int64_t n, int force, int* lanes, int* prefetch, int* persistent) {
  if (cls < CLS_P256 || cls > CLS_ED25519 || n <= 0 || n % WAVE != 0 || !lanes || !prefetch || !persistent) return -1;
  const PointForm f = cls == CLS_ED25519 ? ed_point_form(n) : ec_point_form(cls, n, force != 0);
  *lanes = f.lanes; *prefetch = f.prefetch; *persistent = f.persistent;
  return 0;
}

// cls: CLS_P256 .. CLS_P521; wq: a key-table width of the curve; wpb: waves per
// block, EC_SCALAR_WPB (4) or 1 (the curve's narrowest width only); B: tokens
// per thread, 1..16.  The launch covers [begin, end) of npad padded slots, all
// three multiples of 64, with launch_chain's grid and block for that wpb.
// jobs: npad records in padded order, every wave on one key < nkeys, live lanes
// with alg 7..9 (ES256 / ES384 / ES512), padding lanes with JOB_PAD; only meta
// is read.  valid[nkeys]: DevKey.valid of each key.  sigw: EC_S_ROW + 17 rows x
// npad as prep leaves them (r at row 0, s at row EC_S_ROW); dig: DIG_ROWS x
// npad; status_in: npad bytes.  *exc_count starts at exc_in.
// Out: digs (ec_digit_rows(cls) x npad; 0xA5A5A5A5 wherever the kernel did not
// write), status (npad), *exc_out.  EcArgs is laid out as jg_runtime.cpp does:
// u1w and u2w behind the digit rows, ec_limbs(cls) rows each, stride npad.
// Returns 0; -1 on a bad argument (nothing is launched); -2 on a HIP error.
extern "C" int tk_ec_scalar(int cls, int wq, int wpb, int B, int64_t npad, int64_t begin, int64_t end,
                            const JobDev* jobs, int nkeys, const int32_t* valid, const uint32_t* sigw,
                            const uint32_t* dig, const uint8_t* status_in, int exc_reset, uint32_t exc_in,
                            uint32_t* digs, uint8_t* status, uint32_t* exc_out) {
  if (cls < CLS_P256 || cls > CLS_P521 || !tkes_width_ok(cls, wq, wpb)) return -1;
  if (B < 1 || B > 16) return -1;
  if (npad <= 0 || npad % WAVE != 0 || npad > TKES_MAX_JOBS) return -1;
  if (begin < 0 || begin % WAVE != 0 || end % WAVE != 0 || begin >= end || end > npad) return -1;
  if (!jobs || !valid || !sigw || !dig || !status_in || !digs || !status || !exc_out) return -1;
  if (nkeys <= 0 || nkeys > TKES_MAX_KEYS) return -1;
  if (exc_reset != 0 && exc_reset != 1) return -1;
  for (int64_t w = 0; w < npad; w += WAVE) {
    const int key = job_key(jobs[w]);
    if (key >= nkeys) return -1;
    for (int64_t p = w; p < w + WAVE; ++p) {
      if (job_key(jobs[p]) != key) return -1;                  // the key is wave-uniform
      const int alg = job_alg(jobs[p]);
      if (job_live(jobs[p]) && (alg < 7 || alg > 9)) return -1;
    }
  }

  const size_t np = (size_t)npad;
  const int drows = ec_digit_rows(cls), L = ec_limbs(cls);
  const size_t rows_words = (size_t)(drows + 2 * L) * np;
  std::vector<DevKey> keys((size_t)nkeys);
  for (int k = 0; k < nkeys; ++k) {
    DevKey K{};
    K.kind = 2;
    K.cls = cls;
    K.valid = valid[k] ? 1 : 0;
    K.tab_w = wq;
    keys[(size_t)k] = K;
  }

  JobDev* d_jobs = (JobDev*)tkes_alloc(np * sizeof(JobDev));
  DevKey* d_keys = (DevKey*)tkes_alloc(keys.size() * sizeof(DevKey));
  uint32_t* d_sigw = (uint32_t*)tkes_alloc((size_t)TKES_SIG_ROWS * np * sizeof(uint32_t));
  uint32_t* d_dig = (uint32_t*)tkes_alloc((size_t)DIG_ROWS * np * sizeof(uint32_t));
  uint8_t* d_status = (uint8_t*)tkes_alloc(np);
  uint32_t* d_rows = (uint32_t*)tkes_alloc(rows_words * sizeof(uint32_t));
  uint32_t* d_exc = (uint32_t*)tkes_alloc(sizeof(uint32_t));
  bool ok = d_jobs && d_keys && d_sigw && d_dig && d_status && d_rows && d_exc;
  auto chk = [&](hipError_t e) { ok = ok && e == hipSuccess; };
  if (ok) {
    chk(hipMemcpy(d_jobs, jobs, np * sizeof(JobDev), hipMemcpyHostToDevice));
    chk(hipMemcpy(d_keys, keys.data(), keys.size() * sizeof(DevKey), hipMemcpyHostToDevice));
    chk(hipMemcpy(d_sigw, sigw, (size_t)TKES_SIG_ROWS * np * sizeof(uint32_t), hipMemcpyHostToDevice));
    chk(hipMemcpy(d_dig, dig, (size_t)DIG_ROWS * np * sizeof(uint32_t), hipMemcpyHostToDevice));
    chk(hipMemcpy(d_status, status_in, np, hipMemcpyHostToDevice));
    chk(hipMemcpy(d_exc, &exc_in, sizeof(uint32_t), hipMemcpyHostToDevice));
    // poison: digit rows (and the scratch behind them) the kernel leaves unwritten read back as 0xA5A5A5A5
    chk(hipMemset(d_rows, 0xA5, rows_words * sizeof(uint32_t)));
    chk(hipDeviceSynchronize());
  }
  if (ok) {
    EcArgs ea{};
    ea.jobs = d_jobs; ea.keys = d_keys; ea.keyblob = nullptr;
    ea.sigw = d_sigw; ea.dig = d_dig; ea.status = d_status; ea.verdict_pad = nullptr;
    ea.digs = d_rows;
    ea.u1w = d_rows + (size_t)drows * np;
    ea.u2w = d_rows + (size_t)(drows + L) * np;
    ea.gtab = nullptr; ea.exc_list = nullptr;
    ea.exc_count = d_exc;
    ea.npad = npad; ea.begin = begin; ea.end = end;
    ea.wq = wq; ea.exc_reset = exc_reset; ea.part = EC_FAST;
    const bool launched = cls == CLS_P256   ? tkes_launch_p256(wq, wpb, ea, B)
                          : cls == CLS_P384 ? tkes_launch_p384(wq, wpb, ea, B)
                                            : tkes_launch_p521(wq, wpb, ea, B);
    ok = ok && launched;
    chk(hipGetLastError());
    chk(hipDeviceSynchronize());
  }
  if (ok) {
    chk(hipMemcpy(digs, d_rows, (size_t)drows * np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    chk(hipMemcpy(status, d_status, np, hipMemcpyDeviceToHost));
    chk(hipMemcpy(exc_out, d_exc, sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  for (void* ptr : {(void*)d_jobs, (void*)d_keys, (void*)d_sigw, (void*)d_dig, (void*)d_status, (void*)d_rows,
                    (void*)d_exc})
    if (ptr) (void)hipFree(ptr);
  return ok ? 0 : -2;
}
