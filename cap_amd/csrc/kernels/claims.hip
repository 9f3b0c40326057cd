// claims.hip -- batched scan of the registered claims on gfx950.
//
// The claim checks of cap's Validator.Validate after the signature
// (jwt/jwt.go:103-201) for callers that need the verdict only: one lane per
// token decodes the base64url payload segment and walks the JSON text with the
// scalar state machine of claims.hpp (claims_decide), reading the arena through
// aligned 32-bit words as hash.hip's MemString does -- one word load per four
// characters, never more than seven bytes past the segment (ARENA_SLACK covers
// it).  The resolved Expected (window edges, leeways, expected strings) is
// copied to LDS once per block; the byte compares of a claim value against the
// expected strings are LDS reads.  A wave runs until its longest payload ends.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "claims.hpp"

using namespace jgclaims;

namespace {

// characters [4g, 4g+4) of a segment that starts `shift` bytes into aligned[0]
struct WordSrc {
  const uint32_t* aligned;
  uint32_t shift8;            // 8 * (offset & 3)
  uint32_t cur;               // aligned[g]
  __device__ __forceinline__ uint32_t word(uint32_t g) {
    const uint32_t nxt = aligned[g + 1];
    const uint32_t w = (uint32_t)((((uint64_t)nxt << 32) | cur) >> shift8);
    cur = nxt;
    return w;
  }
};

// One lane's operands (jg_claims_match_args) as the scan reads them: the row of
// the span table and of the numbers that belongs to the lane's job, and the
// operand bytes through aligned words, as WordSrc reads the arena: two word loads
// per four compared bytes, never more than seven bytes past an operand (the
// buffer has ARENA_SLACK behind it).  Nothing is kept in registers here: the
// scan holds the lengths in one dword and a window per column.
struct ArgSrc {
  const uint32_t* words;      // the operand bytes
  const jg_sarg* str;         // the lane's nstr spans
  const int64_t* num;         // the lane's numbers
  uint32_t ns;
  __device__ __forceinline__ uint32_t nstr() const { return ns; }
  __device__ __forceinline__ uint32_t slen(uint32_t c) const { return str[c].len; }
  __device__ __forceinline__ uint32_t word(uint32_t c, uint32_t p) const {
    const uint32_t a = str[c].off + p;
    const uint32_t* q = words + (a >> 2);
    return (uint32_t)((((uint64_t)q[1] << 32) | q[0]) >> (8u * (a & 3u)));
  }
  __device__ __forceinline__ int64_t bound(uint32_t c) const { return num[c]; }
};

// ArgSrc for jg_claims_match_set: the lane's segment too, read again by group in
// any order (WordSrc::word goes forward only), for the compare that confirms a
// set hit.  The same two aligned words per group, so the same seven bytes of slack.
struct SetArgSrc : ArgSrc {
  const uint32_t* aligned;
  uint32_t shift8;
  __device__ __forceinline__ uint32_t peek(uint32_t g) const {
    return (uint32_t)((((uint64_t)aligned[g + 1] << 32) | aligned[g]) >> shift8);
  }
};

constexpr int kBlock = 256;

// the block copies `words` 32-bit words of *src, from word `first` on, to its LDS object *dst
template <class T>
__device__ __forceinline__ void copy_words(T* dst, const T* __restrict__ src, uint32_t first, uint32_t words) {
  static_assert(sizeof(T) % 4 == 0, "copied to LDS by words");
  for (uint32_t k = threadIdx.x; k < words; k += kBlock) ((uint32_t*)dst)[first + k] = ((const uint32_t*)src)[first + k];
}

// the records go out as 16-byte stores: four for a jg_claims, five for a jg_selected
static_assert(sizeof(jg_claims) == 64, "the record is four 16-byte stores");
__device__ __forceinline__ void store_claims(jg_claims* out, const jg_claims& v) {
  uint4* o = (uint4*)out;
  o[0] = make_uint4((uint32_t)v.exp, (uint32_t)((uint64_t)v.exp >> 32), (uint32_t)v.nbf, (uint32_t)((uint64_t)v.nbf >> 32));
  o[1] = make_uint4((uint32_t)v.iat, (uint32_t)((uint64_t)v.iat >> 32), v.iss_off, v.iss_len);
  o[2] = make_uint4(v.sub_off, v.sub_len, v.jti_off, v.jti_len);
  o[3] = make_uint4(v.aud_off, v.aud_len, v.aud_n, v.present);
}
static_assert(sizeof(jg_selected) == 80, "the record is five 16-byte stores");
__device__ __forceinline__ void store_selected(jg_selected* out, const jg_selected& q) {
  uint4* t = (uint4*)out;
  t[0] = make_uint4(q.off[0], q.off[1], q.off[2], q.off[3]);
  t[1] = make_uint4(q.off[4], q.off[5], q.off[6], q.off[7]);
  t[2] = make_uint4(q.len[0], q.len[1], q.len[2], q.len[3]);
  t[3] = make_uint4(q.len[4], q.len[5], q.len[6], q.len[7]);
  t[4] = make_uint4(q.type[0] | (uint32_t)q.type[1] << 8 | (uint32_t)q.type[2] << 16 | (uint32_t)q.type[3] << 24,
                    q.type[4] | (uint32_t)q.type[5] << 8 | (uint32_t)q.type[6] << 16 | (uint32_t)q.type[7] << 24, 0u, 0u);
}

// The body of all ten kernels.  M is the scan's mode.  X is the block's LDS
// copy of the expected side, XS its type:
//   Expect    one for the call, copied whole;
//   Profiles  the call's table (jg_claims_each), copied only as far as it is in
//             use -- the n headers (they follow the two counts) and the pool's
//             used bytes, not all 16 KiB.  Lane i scans against header
//             jobs[i].flags; the lanes of a wave may hold different profiles,
//             which only makes the base of the LDS reads per-lane (their
//             addresses depend on the lane's position in its value already).
// S is the LDS copy of what a selecting mode selects by, SL its type: Select's
// names or, for kPath and kMatch, Paths.  The records stay in registers (fields
// and constant indices only) until they are stored.  Q is the LDS copy of the
// predicates of kMatch and kMatchArgs (PQ: Preds or ArgPreds), which keep no
// record: a byte and a dword per lane.  kMatchArgs also reads the lane's own
// operands, from global memory (ArgSrc).  kMatchSet is kMatchArgs with SetArgPreds
// for PQ: the tables of the call's sets are read from global memory through the
// addresses its headers hold, and the segment a second time (SetArgSrc).
template <int M, class XS, class SL, class PQ = Preds>
__device__ __forceinline__ void claims_body(XS& X, SL* S, const uint8_t* __restrict__ arena,
                                            const jg_cjob* __restrict__ jobs, int64_t n, const XS* __restrict__ expect,
                                            const SL* __restrict__ select, uint8_t* __restrict__ code_out,
                                            jg_claims* __restrict__ vals_out, jg_selected* __restrict__ sel_out,
                                            PQ* Q = nullptr, const PQ* __restrict__ preds = nullptr,
                                            uint32_t* __restrict__ match_out = nullptr,
                                            const uint8_t* __restrict__ arg_bytes = nullptr,
                                            const jg_sarg* __restrict__ arg_str = nullptr,
                                            const int64_t* __restrict__ arg_num = nullptr, uint32_t nstr = 0,
                                            uint32_t nnum = 0) {
  constexpr bool kTable = std::is_same_v<XS, Profiles>;
  uint32_t np = 0;
  if constexpr (kTable) {
    static_assert(offsetof(Profiles, h) == 8 && sizeof(ProfileHeader) % 4 == 0 && offsetof(Profiles, pool) % 4 == 0,
                  "the table is copied by words");
    uint32_t used = expect->pool_used;
    np = expect->n;
    np = np < (uint32_t)JG_MAX_PROFILES ? np : (uint32_t)JG_MAX_PROFILES;       // the runtime resolved it: never taken
    used = used < (uint32_t)JG_PROFILE_POOL_BYTES ? used : (uint32_t)JG_PROFILE_POOL_BYTES;
    copy_words(&X, expect, 0u, (8u + np * (uint32_t)sizeof(ProfileHeader)) / 4u);
    copy_words(&X, expect, offsetof(Profiles, pool) / 4u, (used + 3u) / 4u);
  } else {
    copy_words(&X, expect, 0u, sizeof(Expect) / 4u);
  }
  if constexpr (M >= kSelect) copy_words(S, select, 0u, sizeof(SL) / 4u);
  if constexpr (kPred<M>) copy_words(Q, preds, 0u, sizeof(PQ) / 4u);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const jg_cjob J = jobs[i];
  WordSrc src;
  src.aligned = (const uint32_t*)(arena + (J.off & ~(uint64_t)3));
  src.shift8 = 8u * (uint32_t)(J.off & 3);
  src.cur = src.aligned[0];
  jg_claims v;
  jg_selected q;
  uint32_t bits;
  if constexpr (M == kMatchSet) {
    const ProfileRef E{X, J.flags < np ? J.flags : 0u};
    const SetArgSrc A{{(const uint32_t*)arg_bytes, arg_str + i * nstr, arg_num + i * nnum, nstr}, src.aligned, src.shift8};
    code_out[i] = scan_segment<M>(src, J.len, E, &v, S, &q, Q, &bits, &A);
  } else if constexpr (M == kMatchArgs) {
    const ProfileRef E{X, J.flags < np ? J.flags : 0u};
    const ArgSrc A{(const uint32_t*)arg_bytes, arg_str + i * nstr, arg_num + i * nnum, nstr};
    code_out[i] = scan_segment<M>(src, J.len, E, &v, S, &q, Q, &bits, &A);
  } else if constexpr (kTable) {
    const ProfileRef E{X, J.flags < np ? J.flags : 0u};                         // likewise: checked before the launch
    code_out[i] = scan_segment<M>(src, J.len, E, &v, S, &q, Q, &bits);
  } else {
    code_out[i] = scan_segment<M>(src, J.len, X, &v, S, &q);
  }
  if constexpr (kRec<M>) store_claims(vals_out + i, v);
  if constexpr (kSel<M>) store_selected(sel_out + i, q);
  if constexpr (kPred<M>) match_out[i] = bits;
}

// code_out[i] = the jg_claim_code of jobs[i]
__global__ void __launch_bounds__(kBlock) k_claims_scan(const uint8_t* __restrict__ arena,
                                                        const jg_cjob* __restrict__ jobs, int64_t n,
                                                        const Expect* __restrict__ expect,
                                                        uint8_t* __restrict__ code_out) {
  __shared__ Expect E;
  claims_body<kVerdict, Expect, Select>(E, nullptr, arena, jobs, n, expect, nullptr, code_out, nullptr, nullptr);
}

// k_claims_scan that also keeps what it read: vals_out[i] is token i's record of
// registered claims (jg_claims, 64 bytes)
__global__ void __launch_bounds__(kBlock) k_claims_extract(const uint8_t* __restrict__ arena,
                                                           const jg_cjob* __restrict__ jobs, int64_t n,
                                                           const Expect* __restrict__ expect,
                                                           uint8_t* __restrict__ code_out,
                                                           jg_claims* __restrict__ vals_out) {
  __shared__ Expect E;
  claims_body<kExtract, Expect, Select>(E, nullptr, arena, jobs, n, expect, nullptr, code_out, vals_out, nullptr);
}

// k_claims_extract that also latches where the caller's named top-level
// members lie: sel_out[i] is token i's jg_selected (80 bytes).  The resolved
// names sit in LDS beside the Expected; a depth-1 key is compared with them byte
// by byte from there.
__global__ void __launch_bounds__(kBlock) k_claims_select(const uint8_t* __restrict__ arena,
                                                          const jg_cjob* __restrict__ jobs, int64_t n,
                                                          const Expect* __restrict__ expect,
                                                          const Select* __restrict__ select,
                                                          uint8_t* __restrict__ code_out,
                                                          jg_claims* __restrict__ vals_out,
                                                          jg_selected* __restrict__ sel_out) {
  __shared__ Expect E;
  __shared__ Select S;
  claims_body<kSelect, Expect, Select>(E, &S, arena, jobs, n, expect, select, code_out, vals_out, sel_out);
}

// The three kernels above with a profile per lane (jg_claims_each): the block
// holds the call's Profiles table in LDS instead of one Expect.
__global__ void __launch_bounds__(kBlock) k_claims_scan_each(const uint8_t* __restrict__ arena,
                                                             const jg_cjob* __restrict__ jobs, int64_t n,
                                                             const Profiles* __restrict__ table,
                                                             uint8_t* __restrict__ code_out) {
  __shared__ Profiles T;
  claims_body<kVerdict, Profiles, Select>(T, nullptr, arena, jobs, n, table, nullptr, code_out, nullptr, nullptr);
}

__global__ void __launch_bounds__(kBlock) k_claims_extract_each(const uint8_t* __restrict__ arena,
                                                                const jg_cjob* __restrict__ jobs, int64_t n,
                                                                const Profiles* __restrict__ table,
                                                                uint8_t* __restrict__ code_out,
                                                                jg_claims* __restrict__ vals_out) {
  __shared__ Profiles T;
  claims_body<kExtract, Profiles, Select>(T, nullptr, arena, jobs, n, table, nullptr, code_out, vals_out, nullptr);
}

__global__ void __launch_bounds__(kBlock) k_claims_select_each(const uint8_t* __restrict__ arena,
                                                               const jg_cjob* __restrict__ jobs, int64_t n,
                                                               const Profiles* __restrict__ table,
                                                               const Select* __restrict__ select,
                                                               uint8_t* __restrict__ code_out,
                                                               jg_claims* __restrict__ vals_out,
                                                               jg_selected* __restrict__ sel_out) {
  __shared__ Profiles T;
  __shared__ Select S;
  claims_body<kSelect, Profiles, Select>(T, &S, arena, jobs, n, table, select, code_out, vals_out, sel_out);
}

// k_claims_select_each for members named by path (jg_claims_paths): the resolved
// paths sit in LDS beside the table, and a key at depth d <= JG_PATH_MAX_COMP is
// compared from there with component d of the paths matched that far.
__global__ void __launch_bounds__(kBlock) k_claims_paths_each(const uint8_t* __restrict__ arena,
                                                              const jg_cjob* __restrict__ jobs, int64_t n,
                                                              const Profiles* __restrict__ table,
                                                              const Paths* __restrict__ paths,
                                                              uint8_t* __restrict__ code_out,
                                                              jg_claims* __restrict__ vals_out,
                                                              jg_selected* __restrict__ sel_out) {
  __shared__ Profiles T;
  __shared__ Paths P;
  claims_body<kPath, Profiles, Paths>(T, &P, arena, jobs, n, table, paths, code_out, vals_out, sel_out);
}

// k_claims_scan_each that also answers the caller's predicates on members
// reached by path (jg_claims_match): the resolved paths and predicates sit in LDS
// beside the table; keys are matched as in k_claims_paths_each, and the value a
// path reaches is compared from LDS with the values of the predicates on that
// path.  match_out[i] is the mask of the predicates that hold; no record is kept.
__global__ void __launch_bounds__(kBlock) k_claims_match_each(const uint8_t* __restrict__ arena,
                                                              const jg_cjob* __restrict__ jobs, int64_t n,
                                                              const Profiles* __restrict__ table,
                                                              const Paths* __restrict__ paths,
                                                              const Preds* __restrict__ preds,
                                                              uint8_t* __restrict__ code_out,
                                                              uint32_t* __restrict__ match_out) {
  __shared__ Profiles T;
  __shared__ Paths P;
  __shared__ Preds Q;
  claims_body<kMatch, Profiles, Paths>(T, &P, arena, jobs, n, table, paths, code_out, nullptr, nullptr, &Q, preds,
                                       match_out);
}

// k_claims_match_each whose predicates may also take an operand of the lane's
// own job (jg_claims_match_args) or test a number: the resolved predicates
// (ArgPreds) sit in LDS in the place of Preds; job i's string operands are spans
// arg_str[i * nstr + c] of arg_bytes and are compared from global memory, a
// window of four bytes per column at a time; its numbers are arg_num[i * nnum + c].
__global__ void __launch_bounds__(kBlock) k_claims_match_args(const uint8_t* __restrict__ arena,
                                                              const jg_cjob* __restrict__ jobs, int64_t n,
                                                              const Profiles* __restrict__ table,
                                                              const Paths* __restrict__ paths,
                                                              const ArgPreds* __restrict__ preds,
                                                              const uint8_t* __restrict__ arg_bytes,
                                                              const jg_sarg* __restrict__ arg_str,
                                                              const int64_t* __restrict__ arg_num, uint32_t nstr,
                                                              uint32_t nnum, uint8_t* __restrict__ code_out,
                                                              uint32_t* __restrict__ match_out) {
  __shared__ Profiles T;
  __shared__ Paths P;
  __shared__ ArgPreds Q;
  claims_body<kMatchArgs, Profiles, Paths, ArgPreds>(T, &P, arena, jobs, n, table, paths, code_out, nullptr, nullptr, &Q,
                                                     preds, match_out, arg_bytes, arg_str, arg_num, nstr, nnum);
}

// k_claims_match_args whose predicates may also ask whether a string is a member
// of a resident set (jg_claims_match_set): SetArgPreds sits in LDS in the place
// of ArgPreds, with the headers of the call's sets behind the predicates.
__global__ void __launch_bounds__(kBlock) k_claims_match_set(const uint8_t* __restrict__ arena,
                                                             const jg_cjob* __restrict__ jobs, int64_t n,
                                                             const Profiles* __restrict__ table,
                                                             const Paths* __restrict__ paths,
                                                             const SetArgPreds* __restrict__ preds,
                                                             const uint8_t* __restrict__ arg_bytes,
                                                             const jg_sarg* __restrict__ arg_str,
                                                             const int64_t* __restrict__ arg_num, uint32_t nstr,
                                                             uint32_t nnum, uint8_t* __restrict__ code_out,
                                                             uint32_t* __restrict__ match_out) {
  __shared__ Profiles T;
  __shared__ Paths P;
  __shared__ SetArgPreds Q;
  claims_body<kMatchSet, Profiles, Paths, SetArgPreds>(T, &P, arena, jobs, n, table, paths, code_out, nullptr, nullptr,
                                                       &Q, preds, match_out, arg_bytes, arg_str, arg_num, nstr, nnum);
}

}  // namespace

void launch_claims(const ClaimsLaunch& c, hipStream_t s) {
  if (c.n <= 0) return;
  const dim3 grid((unsigned)((c.n + kBlock - 1) / kBlock)), block(kBlock);
  const auto go = [&](auto kernel, auto... rest) {
    hipLaunchKernelGGL(kernel, grid, block, 0, s, c.arena, c.jobs, c.n, rest...);
  };
  if (c.spreds)
    go(k_claims_match_set, c.table, c.paths, c.spreds, c.arg_bytes, c.arg_str, c.arg_num, c.nstr, c.nnum, c.code_out,
       c.match_out);
  else if (c.apreds)
    go(k_claims_match_args, c.table, c.paths, c.apreds, c.arg_bytes, c.arg_str, c.arg_num, c.nstr, c.nnum, c.code_out,
       c.match_out);
  else if (c.match_out) go(k_claims_match_each, c.table, c.paths, c.preds, c.code_out, c.match_out);
  else if (c.paths) go(k_claims_paths_each, c.table, c.paths, c.code_out, c.vals_out, c.sel_out);
  else if (c.table && c.sel_out) go(k_claims_select_each, c.table, c.select, c.code_out, c.vals_out, c.sel_out);
  else if (c.table && c.vals_out) go(k_claims_extract_each, c.table, c.code_out, c.vals_out);
  else if (c.table) go(k_claims_scan_each, c.table, c.code_out);
  else if (c.sel_out) go(k_claims_select, c.expect, c.select, c.code_out, c.vals_out, c.sel_out);
  else if (c.vals_out) go(k_claims_extract, c.expect, c.code_out, c.vals_out);
  else go(k_claims_scan, c.expect, c.code_out);
}
