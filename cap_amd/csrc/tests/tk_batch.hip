// tk_batch.hip -- TEST INFRASTRUCTURE (libcapjwt_tk.so only, never the
// product path): the dispatch-plan kernels of kernels/batch.hip alone, through
// the production launchers launch_plan_fill, launch_zc_gather, launch_copy and
// launch_scatter, so tests/test_gpu_plan_exact.py can compare every slot they
// write -- and every slot they must leave alone -- with the plain model in
// tests/plan_model.py.  The pipeline behind them only tells accept from reject.
//
// Every hook checks its arguments on the host first and returns -1 without a
// launch when a plan would reach outside its buffers, so a mistake in a test
// cannot read or write out of bounds.  Output buffers carry guard space (TKB_GUARD
// slots behind slot arrays, TKB_GUARD bytes before and after byte buffers), are
// filled with a sentinel (0xA5 bytes: perm 0xA5A5A5A5 would be a negative index,
// so perm is 0x5A5A5A5A) and copied back whole.  All hooks return 0, or -1 on
// bad arguments or a HIP error, and synchronise before they return.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../kernels/batch.hip"   // the kernels are in an anonymous namespace: this TU's own copy

namespace {

constexpr int64_t TKB_GUARD = 64;
constexpr uint64_t TKB_SLACK = 256;          // jg_runtime.cpp ARENA_SLACK
constexpr int64_t TKB_MAX_SLOTS = 1 << 22;   // jobs / padded slots per call
constexpr uint8_t TKB_FILL = 0xA5;
constexpr int32_t TKB_PERM_FILL = 0x5A5A5A5A;

// device buffers of one call, freed on every way out
struct DevBufs {
  std::vector<void*> all;
  template <class T>
  T* get(size_t count) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16)) != hipSuccess) return nullptr;
    all.push_back(p);
    return (T*)p;
  }
  ~DevBufs() {
    for (void* p : all) (void)hipFree(p);
  }
};

bool up(void* d, const void* h, size_t bytes) {
  return bytes == 0 || hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
}
bool down(void* h, const void* d, size_t bytes) {
  return bytes == 0 || hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost) == hipSuccess;
}
bool fill(void* d, int byte, size_t bytes) { return bytes == 0 || hipMemset(d, byte, bytes) == hipSuccess; }
bool ran() { return hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess; }

}  // namespace

// launch_plan_fill on n jobs (device memory, as in the grouped path) over nkeys
// + 1 buckets.  cursor_in[b]: first padded slot of bucket b; pad: [lo, hi) per
// bucket; npad: the slots of the jobs / perm / vpad buffers in front of their
// guards.  jobs_out / perm_out / vpad_out hold npad + 64 slots.  keep == 0: the
// three buffers start as sentinel; keep != 0: they start as the caller's
// jobs_out / perm_out / vpad_out (a buffer reused by the next chunk).
extern "C" int tk_plan_fill(const jg_tok* toks, int64_t n, uint64_t base, const uint8_t* cls_tab, int32_t nkeys,
                            const uint64_t* cursor_in, const int64_t* pad, int64_t npad, JobDev* jobs_out,
                            int32_t* perm_out, uint8_t* vpad_out, uint64_t* cursor_out, int32_t keep) {
  if (n < 0 || n > TKB_MAX_SLOTS || nkeys < 0 || nkeys > 65535 || npad < 0 || npad > TKB_MAX_SLOTS || (n && !toks) ||
      (nkeys && !cls_tab) || !cursor_in || !pad || !jobs_out || !perm_out || !vpad_out || !cursor_out)
    return -1;
  const size_t NB = (size_t)nkeys + 1;
  std::vector<int64_t> total(NB, 0);
  for (int64_t i = 0; i < n; ++i) {
    if (toks[i].key_idx >= nkeys) return -1;
    const int c = toks[i].alg < 16 ? cls_tab[(size_t)toks[i].key_idx * 16 + toks[i].alg] : 0;
    total[c == 0 ? (size_t)nkeys : toks[i].key_idx]++;
  }
  for (size_t b = 0; b < NB; ++b) {
    if (cursor_in[b] > (uint64_t)npad || total[b] > npad - (int64_t)cursor_in[b]) return -1;
    if (pad[2 * b] < 0 || pad[2 * b] > npad || pad[2 * b + 1] > npad) return -1;
  }
  const size_t slots = (size_t)(npad + TKB_GUARD);
  DevBufs D;
  jg_tok* dt = D.get<jg_tok>((size_t)n);
  uint8_t* dc = D.get<uint8_t>((size_t)nkeys * 16);
  unsigned long long* dcur = D.get<unsigned long long>(NB);
  int64_t* dpad = D.get<int64_t>(2 * NB);
  JobDev* dj = D.get<JobDev>(slots);
  int32_t* dp = D.get<int32_t>(slots);
  uint8_t* dv = D.get<uint8_t>(slots);
  if (!dt || !dc || !dcur || !dpad || !dj || !dp || !dv) return -1;
  if (!up(dt, toks, sizeof(jg_tok) * n) || !up(dc, cls_tab, (size_t)nkeys * 16) ||
      !up(dcur, cursor_in, sizeof(uint64_t) * NB) || !up(dpad, pad, sizeof(int64_t) * 2 * NB))
    return -1;
  if (keep) {
    if (!up(dj, jobs_out, sizeof(JobDev) * slots) || !up(dp, perm_out, sizeof(int32_t) * slots) ||
        !up(dv, vpad_out, slots))
      return -1;
  } else {
    std::vector<int32_t> pf(slots, TKB_PERM_FILL);
    if (!fill(dj, TKB_FILL, sizeof(JobDev) * slots) || !up(dp, pf.data(), sizeof(int32_t) * slots) ||
        !fill(dv, TKB_FILL, slots))
      return -1;
  }
  PlanFillArgs a{};
  a.toks = dt;
  a.n = n;
  a.base = base;
  a.cls_tab = dc;
  a.nkeys = nkeys;
  a.cursor = dcur;
  a.pad = dpad;
  a.jobs = dj;
  a.perm = dp;
  a.vpad = dv;
  launch_plan_fill(a, nullptr);
  if (!ran()) return -1;
  if (!down(jobs_out, dj, sizeof(JobDev) * slots) || !down(perm_out, dp, sizeof(int32_t) * slots) ||
      !down(vpad_out, dv, slots) || !down(cursor_out, dcur, sizeof(uint64_t) * NB))
    return -1;
  return 0;
}

// launch_zc_gather over the padded range [begin, end) of npad jobs.  src:
// src_len bytes; its device copy is 16-byte aligned and has ARENA_SLACK zeroed
// bytes behind it.  jobs_out: npad + 64 jobs.  dst_out: 64 guard bytes, dst_len
// bytes (the gather's dst points here, 16-byte aligned), 64 guard bytes.
extern "C" int tk_zc_gather(const uint8_t* src, uint64_t src_len, const JobDev* jobs_in, int64_t npad, int64_t begin,
                            int64_t end, const uint64_t* kbase, const int64_t* kstart, const uint64_t* kstride,
                            int32_t nkeys, uint64_t dst_len, JobDev* jobs_out, uint8_t* dst_out) {
  constexpr uint64_t LIM = uint64_t(1) << 31;
  if (npad < 0 || npad > TKB_MAX_SLOTS || begin < 0 || begin > end || end > npad || nkeys < 0 || nkeys > 65535 ||
      src_len >= LIM || dst_len >= LIM || (src_len && !src) || (npad && !jobs_in) || !jobs_out || !dst_out ||
      (nkeys && (!kbase || !kstart || !kstride)))
    return -1;
  for (int32_t k = 0; k < nkeys; ++k)
    if ((kbase[k] & 15) || (kstride[k] & 15) || kbase[k] > dst_len || kstride[k] > dst_len || kstart[k] < 0 ||
        kstart[k] > npad)
      return -1;
  for (int64_t p = begin; p < end; ++p) {
    const JobDev& jb = jobs_in[p];
    if (!job_live(jb)) continue;
    const int key = job_key(jb);
    if (key >= nkeys || p < kstart[key] || jb.sig_off < jb.off) return -1;
    const uint64_t e = std::max<uint64_t>((uint64_t)jb.off + jb.sig_in_len, (uint64_t)jb.sig_off + job_siglen(jb));
    if (e > src_len) return -1;                                     // the span + ARENA_SLACK inside the source
    const uint64_t lo = jb.off & ~15u, hi = (e + 15) & ~uint64_t(15);
    const uint64_t d0 = kbase[key] + (uint64_t)(p - kstart[key]) * kstride[key];   // < 2^31 + 2^22 * 2^31
    if (hi - lo > kstride[key] || d0 > dst_len || hi - lo > dst_len - d0) return -1;   // the slot inside dst, slots apart
  }
  const size_t slots = (size_t)(npad + TKB_GUARD), dbytes = (size_t)(dst_len + 2 * TKB_GUARD);
  DevBufs D;
  uint8_t* ds = D.get<uint8_t>((size_t)(src_len + TKB_SLACK));
  JobDev* dj = D.get<JobDev>(slots);
  uint64_t* dkb = D.get<uint64_t>((size_t)nkeys);
  int64_t* dks = D.get<int64_t>((size_t)nkeys);
  uint64_t* dkt = D.get<uint64_t>((size_t)nkeys);
  uint8_t* dd = D.get<uint8_t>(dbytes);
  if (!ds || !dj || !dkb || !dks || !dkt || !dd) return -1;
  if (!up(ds, src, (size_t)src_len) || !fill(ds + src_len, 0, TKB_SLACK) || !fill(dj, TKB_FILL, sizeof(JobDev) * slots) ||
      !up(dj, jobs_in, sizeof(JobDev) * npad) || !up(dkb, kbase, sizeof(uint64_t) * nkeys) ||
      !up(dks, kstart, sizeof(int64_t) * nkeys) || !up(dkt, kstride, sizeof(uint64_t) * nkeys) ||
      !fill(dd, TKB_FILL, dbytes))
    return -1;
  ZcGatherArgs a{};
  a.src = ds;
  a.jobs = dj;
  a.begin = begin;
  a.end = end;
  a.kbase = dkb;
  a.kstart = dks;
  a.kstride = dkt;
  a.dst = dd + TKB_GUARD;
  launch_zc_gather(a, nullptr);
  if (!ran()) return -1;
  if (!down(jobs_out, dj, sizeof(JobDev) * slots) || !down(dst_out, dd, dbytes)) return -1;
  return 0;
}

// launch_copy of `bytes` bytes from (a 256-byte-aligned device address +
// src_misalign) to (another + dst_misalign).  dst_out: guard bytes, the bytes
// copied, guard bytes; guard <= 256, misalignments < 256.
extern "C" int tk_copy(const uint8_t* src, uint32_t src_misalign, uint32_t dst_misalign, uint64_t bytes,
                       uint8_t* dst_out, uint32_t guard) {
  if (bytes > (uint64_t(1) << 28) || src_misalign >= 256 || dst_misalign >= 256 || guard > 256 || (bytes && !src) ||
      !dst_out)
    return -1;
  const size_t dbytes = 256 + (size_t)dst_misalign + (size_t)bytes + guard;
  DevBufs D;
  uint8_t* ds = D.get<uint8_t>((size_t)src_misalign + (size_t)bytes);
  uint8_t* dd = D.get<uint8_t>(dbytes);
  if (!ds || !dd || ((uintptr_t)ds & 255) || ((uintptr_t)dd & 255)) return -1;
  if (!up(ds + src_misalign, src, (size_t)bytes) || !fill(dd, TKB_FILL, dbytes)) return -1;
  uint8_t* to = dd + 256 + dst_misalign;
  launch_copy(ds + src_misalign, to, (size_t)bytes, nullptr);
  if (!ran()) return -1;
  if (!down(dst_out, to - guard, (size_t)bytes + 2 * (size_t)guard)) return -1;
  return 0;
}

// launch_scatter of npad padded verdicts through perm into ntok caller slots.
// verdict_out: 64 guard bytes, ntok verdicts, 64 guard bytes.
extern "C" int tk_scatter(const int32_t* perm, const uint8_t* vpad, int64_t npad, int64_t ntok, uint8_t* verdict_out) {
  if (npad < 0 || npad > TKB_MAX_SLOTS || ntok < 0 || ntok > TKB_MAX_SLOTS || (npad && (!perm || !vpad)) ||
      !verdict_out)
    return -1;
  for (int64_t p = 0; p < npad; ++p)
    if (perm[p] >= ntok) return -1;
  const size_t vbytes = (size_t)(ntok + 2 * TKB_GUARD);
  DevBufs D;
  int32_t* dp = D.get<int32_t>((size_t)npad);
  uint8_t* dv = D.get<uint8_t>((size_t)npad);
  uint8_t* dout = D.get<uint8_t>(vbytes);
  if (!dp || !dv || !dout) return -1;
  if (!up(dp, perm, sizeof(int32_t) * npad) || !up(dv, vpad, (size_t)npad) || !fill(dout, TKB_FILL, vbytes)) return -1;
  launch_scatter(dp, dv, dout + TKB_GUARD, npad, nullptr);
  if (!ran()) return -1;
  if (!down(verdict_out, dout, vbytes)) return -1;
  return 0;
}
