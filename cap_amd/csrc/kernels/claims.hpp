// claims.hpp -- the registered-claims scan: decision function, its resolved
// Expected, and the launch interface of k_claims_scan (claims.hip).
//
// claims_decide() reads one token's base64url payload segment and returns the
// jg_claim_code that Validator's claim checks (jwt/jwt.go:103-201, after the
// signature and the alg header) would end in -- or JG_CL_HOST whenever it
// cannot prove that: the scan is conservative, every code other than HOST is
// exactly the host path's outcome.  What is decided (DESIGN.md "Claims scan"):
//   - the segment is canonical unpadded base64url;
//   - the text is one JSON object, well formed to the end, depth <= 32, only
//     space/tab/LF/CR as whitespace, no backslash and no control byte in any
//     string, numbers of at most 17 bytes without an exponent;
//   - no top-level key holds a byte >= 0x80, no registered field is named
//     twice (in any casing);
//   - iss/sub/jti are null or ASCII strings, aud an ASCII string or an array of
//     them, exp/nbf/iat null or integers -?(0|[1-9][0-9]{0,14}) other than -0.
// The function is __host__ __device__ with the segment fetch abstracted (Src:
// `uint32_t word(uint32_t g)` = characters [4g, 4g+4) little-endian), so the
// CPU tests compile the very code the kernel runs.  All state is scalar: no
// arrays indexed at run time, nothing that would go to scratch.
//
// claims_extract() is the same scan with extraction switched on at compile
// time (ScanT<kExtract>): the same code, plus a jg_claims record of the
// registered claims -- the dates as numbers, iss / sub / jti / aud as byte spans
// into the decoded payload.  ScanT<kVerdict> is the verdict-only scan, unchanged.
//
// claims_select() is a third mode of the same scan (ScanT<kSelect>): the code
// and the record of claims_extract, plus a jg_selected record of up to
// JG_MAX_SELECT top-level members the caller names (Select, in LDS beside
// Expect): a candidate mask over the names is armed when a depth-1 key opens,
// narrowed per key byte and resolved at the closing quote; the value's first
// byte latches the slot's offset and type, its end the length.
//
// claims_paths_each() is a fourth mode (ScanT<kPath>): claims_select's outputs
// for members named by a path of up to JG_PATH_MAX_COMP keys (Paths, in LDS
// beside the profile table): component j is matched at depth j inside the object
// that components 1..j-1 opened.
//
// claims_match_each() is a fifth mode (ScanT<kMatch>): the path matcher of
// kPath without any record, and in the place of the spans a mask of the
// caller's predicates (Preds, in LDS beside the paths) that hold on the values
// the paths reach: a candidate mask over the predicates' values is armed by the
// value's first byte, narrowed per byte and resolved at the closing quote, as
// `cand` is for the expected strings.
//
// claims_match_args() is a sixth mode (ScanT<kMatchArgs>): kMatch whose
// predicates (ArgPreds, in the place of Preds) may compare a string with an
// operand of the token's own -- read from global memory through a window of four
// bytes per column, its length kept in a byte of one dword -- or a number with a
// bound, the token's own or the list's: decided on integers of at most 15 digits
// and left to the host (the one code a predicate changes) on any other number.
// The same mode serves jg_claims_match_hash: IS_STRING is one more per-path mask
// that the opening quote of the selected value sets, and EQUALS_HASH resolves to
// EQUALS_ARG on a string column whose operand k_hash_operand wrote
// (hash_operand.hpp), so the scan itself knows nothing about hashes.
//
// claims_match_set() is a seventh mode (ScanT<kMatchSet>): kMatchArgs whose
// predicates (SetArgPreds: ArgPreds and, behind it, SetPreds) may also ask whether
// a string, or a string element of an array, is a member of a resident set
// (claim_set.hpp): the string is hashed as it goes by -- one running hash, seeded
// per set only where it is finalised -- and looked up at its closing quote; a slot
// whose hash and length agree is confirmed against the payload, read again from
// the decoded position of the string's first byte, which this mode keeps.
//
// The expected side is a template parameter of the scan (EX: slen / sbyte / auds
// and the window's edges).  Expect is one; ProfileRef, one profile of a
// Profiles table picked per token, is the other: claims_decide_each,
// claims_extract_each and claims_select_each are the same three scans for a
// batch whose tokens are held to different Expecteds.
#pragma once
#include <cstdint>
#include <type_traits>

#include "../../../include/jg.h"
#include "claim_set.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JG_CL_HD __host__ __device__ __forceinline__
#else
#define JG_CL_HD inline
#endif

namespace jgclaims {

constexpr int kStrings = 3 + JG_MAX_AUD;          // issuer, subject, id, audiences
constexpr int64_t kUnixToInternal = 62135596800LL;   // time.unixToInternal
constexpr int64_t kNsPerSec = 1000000000LL;

// One resolved Expected as the scan reads it (a device buffer copied to LDS).
struct Expect {
  int64_t hi_sec;           // now + skew, seconds since year 1 (Time.Add)
  int64_t lo_sec;           // now - skew
  int32_t lo_ns;            // ... and its nanoseconds (the later edge is compared at whole seconds)
  uint32_t naud;
  int64_t exp_leeway_s, nbf_leeway_s;
  uint16_t len[kStrings];   // 0 issuer, 1 subject, 2 id, 3.. audiences
  uint16_t off[kStrings];
  uint8_t bytes[JG_EXPECT_MAX_BYTES];
  // how the scan reads an expected side (Expect here, ProfileRef below)
  JG_CL_HD uint32_t slen(uint32_t k) const { return len[k]; }
  JG_CL_HD uint32_t sbyte(uint32_t k, uint32_t pos) const { return bytes[off[k] + pos]; }
  JG_CL_HD uint32_t auds() const { return naud; }
  JG_CL_HD int64_t hi() const { return hi_sec; }
  JG_CL_HD int64_t lo() const { return lo_sec; }
  JG_CL_HD int32_t lons() const { return lo_ns; }
  JG_CL_HD int64_t exp_leeway() const { return exp_leeway_s; }
  JG_CL_HD int64_t nbf_leeway() const { return nbf_leeway_s; }
};

// time.Time.Add of a duration to (sec, nsec): Go's truncating division
JG_CL_HD void time_add(int64_t sec, int64_t nsec, int64_t d, int64_t* osec, int32_t* onsec) {
  int64_t ds = d / kNsPerSec;
  int64_t n2 = nsec + d % kNsPerSec;
  if (n2 >= kNsPerSec) { ++ds; n2 -= kNsPerSec; }
  else if (n2 < 0) { --ds; n2 += kNsPerSec; }
  *osec = sec + ds;
  *onsec = (int32_t)n2;
}

// What resolve() and resolve_profiles() share: one jg_expect into H (an Expect
// or a ProfileHeader: the same fields) -- the window's edges, the leeways and the
// 19 lengths and offsets -- with its string bytes copied to dst from *o on, which
// moves past them.  An empty string's offset is the running one, or 0 with
// empty_at_zero.  False, before anything is written: more than JG_MAX_AUD
// audiences, a bad now, strings over JG_EXPECT_MAX_BYTES in total or past `room`.
template <class H>
inline bool resolve_one(const jg_expect& x, H* h, uint8_t* dst, uint32_t* o, uint32_t room, bool empty_at_zero) {
  if (x.naud > JG_MAX_AUD || x.now_nsec >= (uint32_t)kNsPerSec) return false;
  uint64_t total = (uint64_t)x.iss_len + x.sub_len + x.jti_len;
  for (uint32_t k = 0; k < x.naud; ++k) total += x.aud_len[k];
  if (total > JG_EXPECT_MAX_BYTES || (total && !x.strs) || *o + total > room) return false;
  int32_t hi_ns;
  time_add(x.now_sec + kUnixToInternal, x.now_nsec, x.skew_ns, &h->hi_sec, &hi_ns);
  time_add(x.now_sec + kUnixToInternal, x.now_nsec, -x.skew_ns, &h->lo_sec, &h->lo_ns);
  h->naud = x.naud;
  h->exp_leeway_s = x.exp_leeway_s;
  h->nbf_leeway_s = x.nbf_leeway_s;
  uint32_t so = 0;                                   // within x.strs
  for (int k = 0; k < kStrings; ++k) {
    const uint32_t l = k == 0 ? x.iss_len : k == 1 ? x.sub_len : k == 2 ? x.jti_len
                       : (uint32_t)(k - 3) < x.naud ? x.aud_len[k - 3] : 0u;
    h->len[k] = (uint16_t)l;
    h->off[k] = (uint16_t)(l || !empty_at_zero ? *o : 0u);
    for (uint32_t b = 0; b < l; ++b) dst[*o + b] = x.strs[so + b];
    *o += l;
    so += l;
  }
  return true;
}

// Fills *E from the ABI's jg_expect.  False: more than JG_MAX_AUD audiences,
// strings over JG_EXPECT_MAX_BYTES in total (or one over 65535), a bad now.
inline bool resolve(const jg_expect& x, Expect* E) {
  uint32_t o = 0;
  if (!resolve_one(x, E, E->bytes, &o, JG_EXPECT_MAX_BYTES, false)) return false;
  for (uint32_t b = o; b < JG_EXPECT_MAX_BYTES; ++b) E->bytes[b] = 0;
  return true;
}

// Up to JG_MAX_PROFILES resolved Expecteds for one call (jg_claims_each): the
// per-token form of Expect.  A fixed-size header per profile and one pool of
// JG_PROFILE_POOL_BYTES string bytes that the headers' offsets point into --
// offsets, never pointers: the kernel holds the table in LDS and a pointer kept
// there would be read back as a generic one.  64 x 120 B + 8 KiB is under 16 KiB
// per block, where one Expect per profile would be 4216 B each.
struct ProfileHeader {
  int64_t hi_sec, lo_sec;
  int64_t exp_leeway_s, nbf_leeway_s;
  int32_t lo_ns;
  uint32_t naud;
  uint16_t len[kStrings];   // as Expect's
  uint16_t off[kStrings];   // into Profiles::pool
  uint32_t pad_;
};
struct Profiles {
  uint32_t n;               // headers in use
  uint32_t pool_used;       // pool bytes in use
  ProfileHeader h[JG_MAX_PROFILES];
  uint8_t pool[JG_PROFILE_POOL_BYTES];
};
static_assert(sizeof(ProfileHeader) == 120, "a profile header is 120 bytes");
static_assert(sizeof(Profiles) == 8 + 120 * JG_MAX_PROFILES + JG_PROFILE_POOL_BYTES, "no padding in the table");
static_assert(JG_PROFILE_POOL_BYTES <= 65536, "pool offsets are 16 bits");

// Fills *T from n jg_expect.  False: n == 0 or over JG_MAX_PROFILES, a profile
// resolve() refuses, strings over JG_PROFILE_POOL_BYTES in total.  Header p and
// its pool bytes hold what resolve(x[p]) puts into an Expect; the unused
// headers and the unused pool tail are zero.
inline bool resolve_profiles(const jg_expect* x, uint32_t n, Profiles* T) {
  if (!x || n == 0 || n > JG_MAX_PROFILES) return false;
  uint32_t o = 0;
  for (uint32_t p = 0; p < n; ++p) {
    // an empty string is never read: its offset 0 keeps every offset in 16 bits
    if (!resolve_one(x[p], &T->h[p], T->pool, &o, JG_PROFILE_POOL_BYTES, true)) return false;
    T->h[p].pad_ = 0;
  }
  for (uint32_t p = n; p < JG_MAX_PROFILES; ++p) T->h[p] = ProfileHeader{};
  for (uint32_t b = o; b < JG_PROFILE_POOL_BYTES; ++b) T->pool[b] = 0;
  T->n = n;
  T->pool_used = o;
  return true;
}

// Profile p of a table as the scan reads an expected side: Expect's accessors
// with a per-lane base.  The table is held by reference (in the kernel: the
// block's LDS copy), so every read is an indexed read of that object.
struct ProfileRef {
  const Profiles& T;
  uint32_t p;
  JG_CL_HD uint32_t slen(uint32_t k) const { return T.h[p].len[k]; }
  JG_CL_HD uint32_t sbyte(uint32_t k, uint32_t pos) const { return T.pool[T.h[p].off[k] + pos]; }
  JG_CL_HD uint32_t auds() const { return T.h[p].naud; }
  JG_CL_HD int64_t hi() const { return T.h[p].hi_sec; }
  JG_CL_HD int64_t lo() const { return T.h[p].lo_sec; }
  JG_CL_HD int32_t lons() const { return T.h[p].lo_ns; }
  JG_CL_HD int64_t exp_leeway() const { return T.h[p].exp_leeway_s; }
  JG_CL_HD int64_t nbf_leeway() const { return T.h[p].nbf_leeway_s; }
};

// The caller's claim names as the selecting scan reads them (a device buffer
// copied to LDS beside Expect)
struct Select {
  uint32_t n;
  uint16_t len[JG_MAX_SELECT];
  uint16_t off[JG_MAX_SELECT];
  uint8_t bytes[JG_MAX_SELECT * JG_SELECT_NAME_MAX];
};

// A claim name as resolve_select() and resolve_paths() take one: 1 to
// JG_SELECT_NAME_MAX bytes, each in 0x20..0x7e and neither a quote nor a backslash
inline bool name_byte_ok(uint8_t c) { return c >= 0x20u && c <= 0x7eu && c != '"' && c != '\\'; }
inline bool copy_name(const uint8_t* src, uint32_t l, uint8_t* dst) {
  if (!src || l == 0 || l > JG_SELECT_NAME_MAX) return false;
  for (uint32_t b = 0; b < l; ++b) {
    if (!name_byte_ok(src[b])) return false;
    dst[b] = src[b];
  }
  return true;
}

// Fills *S from the ABI's jg_select.  False: more than JG_MAX_SELECT names, a
// name copy_name() refuses, two equal names.
inline bool resolve_select(const jg_select& x, Select* S) {
  if (x.n > JG_MAX_SELECT) return false;
  uint32_t o = 0;
  for (uint32_t k = 0; k < JG_MAX_SELECT; ++k) {
    const uint32_t l = k < x.n ? x.name_len[k] : 0u;
    if (k < x.n && !copy_name(x.names ? x.names + o : nullptr, l, S->bytes + o)) return false;
    S->len[k] = (uint16_t)l;
    S->off[k] = (uint16_t)o;
    for (uint32_t j = 0; j < k; ++j) {
      if (S->len[j] != l || l == 0) continue;
      uint32_t b = 0;
      while (b < l && S->bytes[S->off[j] + b] == S->bytes[o + b]) ++b;
      if (b == l) return false;
    }
    o += l;
  }
  for (uint32_t b = o; b < sizeof S->bytes; ++b) S->bytes[b] = 0;
  S->n = x.n;
  return true;
}

// The caller's claim paths as the path-selecting scan reads them (a device
// buffer copied to LDS beside the profile table).  Masks over the paths hold
// path k at bit 2k, the position of its field in the scan's matched depths.
struct Paths {
  uint32_t n;
  uint32_t ge[JG_PATH_MAX_COMP];                      // ge[d-1]: the paths with at least d components
  uint8_t ncomp[JG_MAX_PATHS];
  uint8_t len[JG_MAX_PATHS][JG_PATH_MAX_COMP];
  uint16_t off[JG_MAX_PATHS][JG_PATH_MAX_COMP];       // into pool
  uint8_t pool[JG_MAX_PATHS * JG_PATH_MAX_COMP * JG_SELECT_NAME_MAX];
};
static_assert(sizeof(Paths) == 4 + 16 + 8 + 32 + 64 + 2048, "no padding in the paths");
static_assert(JG_MAX_PATHS == JG_MAX_SELECT && JG_PATH_MAX_COMP == 4, "a path per jg_selected slot, two bits of matched depth");

// Fills *P from the ABI's jg_paths.  False: more than JG_MAX_PATHS paths, a path
// of no or more than JG_PATH_MAX_COMP components, a component copy_name()
// refuses, two equal paths.
inline bool resolve_paths(const jg_paths& x, Paths* P) {
  if (x.n > JG_MAX_PATHS) return false;
  *P = Paths{};
  uint32_t o = 0;
  for (uint32_t k = 0; k < x.n; ++k) {
    const uint32_t nc = x.ncomp[k];
    if (nc == 0 || nc > JG_PATH_MAX_COMP || !x.names) return false;
    P->ncomp[k] = (uint8_t)nc;
    for (uint32_t d = 0; d < nc; ++d) {
      const uint32_t l = x.comp_len[k][d];
      if (!copy_name(x.names + o, l, P->pool + o)) return false;
      P->len[k][d] = (uint8_t)l;
      P->off[k][d] = (uint16_t)o;
      o += l;
      P->ge[d] |= 1u << (2u * k);
    }
    for (uint32_t j = 0; j < k; ++j) {
      if (P->ncomp[j] != nc) continue;
      bool same = true;
      for (uint32_t d = 0; d < nc && same; ++d) {
        same = P->len[j][d] == P->len[k][d];
        for (uint32_t b = 0; same && b < P->len[k][d]; ++b)
          same = P->pool[P->off[j][d] + b] == P->pool[P->off[k][d] + b];
      }
      if (same) return false;
    }
  }
  P->n = x.n;
  return true;
}

// The caller's predicates as the matching scan reads them (a device buffer
// copied to LDS beside the profile table and the paths).  Masks over the
// predicates hold predicate k at bit k.  Per path: every predicate on it -- what a
// member that replaces the path's value clears -- and those the first byte of its
// value arms, split by operator.
struct Preds {
  uint32_t n;
  uint16_t all[JG_MAX_PATHS];                         // every predicate on the path
  uint16_t present[JG_MAX_PATHS];                     // PRESENT: set when the value begins
  uint16_t str[JG_MAX_PATHS];                         // EQUALS and HAS_WORD: armed by a string
  uint16_t word[JG_MAX_PATHS];                        // HAS_WORD alone: armed again after a space
  uint16_t elem[JG_MAX_PATHS];                        // HAS_ELEMENT: armed by a string element of the array
  uint8_t op[JG_MAX_PRED];
  uint8_t len[JG_MAX_PRED];
  uint16_t off[JG_MAX_PRED];                          // into pool
  uint8_t pool[JG_MAX_PRED * JG_PRED_VALUE_MAX];
};
static_assert(sizeof(Preds) == 4 + 5 * 16 + 16 + 16 + 32 + 1024, "no padding in the predicates");
static_assert(JG_MAX_PRED <= 16 && JG_PRED_VALUE_MAX <= 255, "a 16-bit mask per path, a byte per length");

// Fills *Q from the ABI's jg_preds, for the resolved paths P of the same call.
// False: more than JG_MAX_PRED predicates, a path index past P.n, an unknown
// operator, a length outside the operator's range (EQUALS 0..JG_PRED_VALUE_MAX,
// HAS_WORD and HAS_ELEMENT 1..JG_PRED_VALUE_MAX, PRESENT 0), a value byte
// name_byte_ok() refuses, a space in a HAS_WORD value, two identical predicates.
inline bool resolve_preds(const jg_preds& x, const Paths& P, Preds* Q) {
  if (x.n > JG_MAX_PRED) return false;
  *Q = Preds{};
  uint8_t path[JG_MAX_PRED] = {};
  uint32_t o = 0;
  for (uint32_t k = 0; k < x.n; ++k) {
    const uint32_t p = x.path[k], op = x.op[k], l = x.value_len[k];
    if (p >= P.n || op < JG_PRED_EQUALS || op > JG_PRED_PRESENT) return false;
    const uint32_t lo = op == JG_PRED_EQUALS || op == JG_PRED_PRESENT ? 0u : 1u;
    const uint32_t hi = op == JG_PRED_PRESENT ? 0u : (uint32_t)JG_PRED_VALUE_MAX;
    if (l < lo || l > hi || (l && !x.values)) return false;
    for (uint32_t b = 0; b < l; ++b) {
      const uint8_t c = x.values[o + b];
      if (!name_byte_ok(c) || (op == JG_PRED_HAS_WORD && c == 0x20u)) return false;
      Q->pool[o + b] = c;
    }
    path[k] = (uint8_t)p;
    Q->op[k] = (uint8_t)op;
    Q->len[k] = (uint8_t)l;
    Q->off[k] = (uint16_t)o;
    for (uint32_t j = 0; j < k; ++j) {
      if (path[j] != p || Q->op[j] != op || Q->len[j] != l) continue;
      uint32_t b = 0;
      while (b < l && Q->pool[Q->off[j] + b] == Q->pool[o + b]) ++b;
      if (b == l) return false;
    }
    const uint16_t bit = (uint16_t)(1u << k);
    Q->all[p] |= bit;
    if (op == JG_PRED_PRESENT) Q->present[p] |= bit;
    if (op == JG_PRED_EQUALS || op == JG_PRED_HAS_WORD) Q->str[p] |= bit;
    if (op == JG_PRED_HAS_WORD) Q->word[p] |= bit;
    if (op == JG_PRED_HAS_ELEMENT) Q->elem[p] |= bit;
    o += l;
  }
  Q->n = x.n;
  return true;
}

// The predicates of jg_claims_match_args as its scan reads them: Preds' fields
// under Preds' names (the scan reads either through the same code), and for the
// five ops only that entry takes: the column of a predicate whose operand is the
// lane's own, the constant numeric bounds, and per path the numeric predicates.
// An ARG or numeric predicate has no bytes in the pool (len 0); EQUALS_ARG is in
// `str` like EQUALS, so a string arms it.
struct ArgPreds {
  int64_t bound[JG_MAX_PRED];                         // NUM_GE / NUM_LE: B
  uint32_t n;
  uint16_t all[JG_MAX_PATHS], present[JG_MAX_PATHS], str[JG_MAX_PATHS], word[JG_MAX_PATHS], elem[JG_MAX_PATHS];
  uint16_t num[JG_MAX_PATHS];                         // the numeric predicates on the path
  uint16_t isstr[JG_MAX_PATHS];                       // IS_STRING (jg_claims_match_hash): set when the value begins with a quote
  uint16_t arg;                                       // the operand is the lane's: EQUALS_ARG, NUM_GE_ARG, NUM_LE_ARG
  uint16_t le;                                        // NUM_LE and NUM_LE_ARG; the other numeric ones are >=
  uint8_t op[JG_MAX_PRED];
  uint8_t len[JG_MAX_PRED];
  uint8_t col[JG_MAX_PRED];                           // the column of an ARG predicate
  uint16_t off[JG_MAX_PRED];
  uint8_t pool[JG_MAX_PRED * JG_PRED_VALUE_MAX];
};
static_assert(sizeof(ArgPreds) == 128 + 4 + 7 * 16 + 4 + 3 * 16 + 32 + 1024 && sizeof(ArgPreds) % 8 == 0,
              "no padding in the predicates with operands");
static_assert(JG_MAX_ARGS == 4 && JG_PRED_VALUE_MAX <= 255, "four operand lengths in one dword");
static_assert(JG_MAX_HASH_ARGS <= JG_MAX_ARGS, "a hashed column is a string column of the kernel");

// The set side of jg_claims_match_set's predicates, behind ArgPreds in LDS: per
// path the predicates a string arms (IN_SET) and those a string element of the
// path's array arms (ELEMENT_IN_SET), per predicate the set of the call it asks,
// and the call's sets as a lookup reads them.  The two pointers are device
// addresses kept as integers: they are read back from LDS and used as they are.
struct SetHeader {
  uint64_t slots, pool;                               // jgset::Slot[mask + 1], the pool's dwords
  uint32_t mask, maxprobe, seed, n;                   // n is not read by the scan: it keeps the header 32 bytes and self-describing
};
struct SetPreds {
  uint16_t inset[JG_MAX_PATHS];
  uint16_t elemset[JG_MAX_PATHS];
  uint8_t set[JG_MAX_PRED];                           // the set index of a set predicate
  uint32_t nsets, pad_;
  SetHeader h[JG_MAX_SETS];
};
struct SetArgPreds : ArgPreds {
  SetPreds sets;
};
static_assert(sizeof(SetHeader) == 32 && sizeof(SetPreds) == 16 + 16 + 16 + 8 + 32 * JG_MAX_SETS, "no padding in the set side");
static_assert(sizeof(SetArgPreds) == sizeof(ArgPreds) + sizeof(SetPreds), "the set side lies right behind the predicates");

// Fills *Q from the ABI's jg_preds as jg_claims_match_args reads it, for the
// resolved paths P and the column counts of the same call.  Ops 1..4 are held to
// resolve_preds' rules.  False also for: a column count over JG_MAX_ARGS, an
// EQUALS_ARG or NUM_*_ARG whose value is not one byte below its column count, a
// NUM_GE / NUM_LE whose value is not eight bytes (B, little-endian), two identical
// predicates (for an ARG one: the same path, op and column).
// With hash_ops (jg_claims_match_hash) the list may also hold JG_PRED_EQUALS_HASH
// -- one value byte, the hash column h < nhash; resolved to EQUALS_ARG on string
// column nstr + h, where the device writes that job's operand -- and
// JG_PRED_IS_STRING (no value).  False also for: nhash over JG_MAX_HASH_ARGS,
// nstr + nhash over JG_MAX_ARGS, two EQUALS_HASH of one path and column, two
// IS_STRING of one path.
// With SP (jg_claims_match_set) the list may also hold JG_PRED_IN_SET and
// JG_PRED_ELEMENT_IN_SET -- one value byte, the set index < nsets -- whose masks
// and indices go to *SP (its headers are the caller's to fill).  False also for:
// nsets over JG_MAX_SETS, two of them of one path, op and set.
inline bool resolve_arg_preds(const jg_preds& x, const Paths& P, uint32_t nstr, uint32_t nnum, ArgPreds* Q,
                              bool hash_ops = false, uint32_t nhash = 0, uint32_t nsets = 0, SetPreds* SP = nullptr) {
  if (x.n > JG_MAX_PRED || nstr > JG_MAX_ARGS || nnum > JG_MAX_ARGS) return false;
  if (nsets > JG_MAX_SETS || (nsets && !SP)) return false;
  if (SP) {
    *SP = SetPreds{};
    SP->nsets = nsets;
  }
  if (nhash > JG_MAX_HASH_ARGS || nstr + nhash > JG_MAX_ARGS || (nhash && !hash_ops)) return false;
  *Q = ArgPreds{};
  uint8_t path[JG_MAX_PRED] = {}, rawop[JG_MAX_PRED] = {};
  uint32_t vlen[JG_MAX_PRED] = {}, voff[JG_MAX_PRED] = {};        // within x.values
  uint32_t o = 0, po = 0;                                         // within x.values, within the pool
  for (uint32_t k = 0; k < x.n; ++k) {
    const uint32_t p = x.path[k], op = x.op[k], l = x.value_len[k];
    if (p >= P.n || op < JG_PRED_EQUALS ||
        op > (SP ? (uint32_t)JG_PRED_ELEMENT_IN_SET : hash_ops ? (uint32_t)JG_PRED_IS_STRING : (uint32_t)JG_PRED_NUM_LE_ARG))
      return false;
    const bool setop = op >= JG_PRED_IN_SET;
    const bool konst = op <= JG_PRED_PRESENT;
    const bool hash = op == JG_PRED_EQUALS_HASH, isstr = op == JG_PRED_IS_STRING;
    const bool arg = op == JG_PRED_EQUALS_ARG || op == JG_PRED_NUM_GE_ARG || op == JG_PRED_NUM_LE_ARG || hash;
    const bool num = op >= JG_PRED_NUM_GE && op <= JG_PRED_NUM_LE_ARG;
    const uint32_t lo = konst ? (op == JG_PRED_EQUALS || op == JG_PRED_PRESENT ? 0u : 1u) : arg || setop ? 1u : isstr ? 0u : 8u;
    const uint32_t hi = konst ? (op == JG_PRED_PRESENT ? 0u : (uint32_t)JG_PRED_VALUE_MAX) : lo;
    if (l < lo || l > hi || (l && !x.values)) return false;
    if (konst) {
      for (uint32_t b = 0; b < l; ++b) {
        const uint8_t c = x.values[o + b];
        if (!name_byte_ok(c) || (op == JG_PRED_HAS_WORD && c == 0x20u)) return false;
        Q->pool[po + b] = c;
      }
      Q->len[k] = (uint8_t)l;
      Q->off[k] = (uint16_t)po;
      po += l;
    } else if (arg) {
      if (x.values[o] >= (hash ? nhash : op == JG_PRED_EQUALS_ARG ? nstr : nnum)) return false;
      Q->col[k] = (uint8_t)(x.values[o] + (hash ? nstr : 0u));
    } else if (setop) {
      if (x.values[o] >= nsets) return false;
      SP->set[k] = x.values[o];
    } else if (!isstr) {
      uint64_t b8 = 0;
      for (uint32_t b = 0; b < 8u; ++b) b8 |= (uint64_t)x.values[o + b] << (8u * b);
      Q->bound[k] = (int64_t)b8;
    }
    path[k] = (uint8_t)p;
    rawop[k] = (uint8_t)op;
    Q->op[k] = (uint8_t)(hash ? (uint32_t)JG_PRED_EQUALS_ARG : op);   // the scan's form
    vlen[k] = l;
    voff[k] = o;
    for (uint32_t j = 0; j < k; ++j) {
      if (path[j] != p || rawop[j] != op || vlen[j] != l) continue;
      uint32_t b = 0;
      while (b < l && x.values[voff[j] + b] == x.values[o + b]) ++b;
      if (b == l) return false;
    }
    const uint16_t bit = (uint16_t)(1u << k);
    Q->all[p] |= bit;
    if (op == JG_PRED_PRESENT) Q->present[p] |= bit;
    if (op == JG_PRED_EQUALS || op == JG_PRED_HAS_WORD || op == JG_PRED_EQUALS_ARG || hash) Q->str[p] |= bit;
    if (op == JG_PRED_HAS_WORD) Q->word[p] |= bit;
    if (op == JG_PRED_HAS_ELEMENT) Q->elem[p] |= bit;
    if (num) Q->num[p] |= bit;
    if (isstr) Q->isstr[p] |= bit;
    if (op == JG_PRED_IN_SET) SP->inset[p] |= bit;
    if (op == JG_PRED_ELEMENT_IN_SET) SP->elemset[p] |= bit;
    if (arg) Q->arg |= bit;
    if (op == JG_PRED_NUM_LE || op == JG_PRED_NUM_LE_ARG) Q->le |= bit;
    o += l;
  }
  Q->n = x.n;
  return true;
}

// One job's operands as jg_claims_match_args checks them before the launch:
// every string operand within `bytes`, at most JG_PRED_VALUE_MAX bytes, each a
// value's byte (name_byte_ok).  False: job i's operands are refused.
inline bool arg_operands_ok(const jg_args& a, size_t i) {
  for (uint32_t c = 0; c < a.nstr; ++c) {
    const jg_sarg& s = a.str[i * a.nstr + c];
    if (s.len > JG_PRED_VALUE_MAX || s.off > a.bytes_len || s.len > a.bytes_len - s.off) return false;
    for (uint32_t b = 0; b < s.len; ++b)
      if (!name_byte_ok(a.bytes[s.off + b])) return false;
  }
  return true;
}

// One job's sources as jg_claims_match_hash checks them before the launch: every
// span within `bytes`, at most JG_HASH_SRC_MAX bytes, a family in 0..3.  False:
// job i's sources are refused.
inline bool hash_sources_ok(const jg_hargs& h, size_t i) {
  for (uint32_t c = 0; c < h.nhash; ++c) {
    const jg_hsrc& s = h.src[i * h.nhash + c];
    if (s.fam > JG_SHA512 || s.len > JG_HASH_SRC_MAX || s.off > h.bytes_len || s.len > h.bytes_len - s.off) return false;
  }
  return true;
}

// No operands: what the modes without them hand the scan
struct NoArgs {};

enum : uint32_t {
  ST_START, ST_VALUE, ST_ARR_FIRST, ST_OBJ_FIRST, ST_OBJ_KEY, ST_COLON, ST_AFTER, ST_STR,
  ST_NUM_MINUS, ST_NUM_ZERO, ST_NUM_INT, ST_NUM_DOT, ST_NUM_FRAC, ST_LIT, ST_DONE
};
// jwt.Claims fields in the order of the checks' fields table (bit f of `seen`)
enum : uint32_t { F_NONE = 0, F_ISS = 1, F_SUB = 2, F_JTI = 3, F_AUD = 4, F_EXP = 5, F_NBF = 6, F_IAT = 7 };

JG_CL_HD uint32_t field_of(uint32_t kw) {            // three upper-cased key bytes
  return kw == 0x495353u ? F_ISS : kw == 0x535542u ? F_SUB : kw == 0x4a5449u ? F_JTI : kw == 0x415544u ? F_AUD
       : kw == 0x455850u ? F_EXP : kw == 0x4e4246u ? F_NBF : kw == 0x494154u ? F_IAT : (uint32_t)F_NONE;
}

// What the extracting form (claims_extract) keeps beside the verdict's state:
// where the registered strings lie in the decoded payload, and which fields the
// payload names with a non-null value.  Scalars, latched with selects.
struct Extract {
  uint32_t dpos = 0;                // decoded position of the byte step() is reading: 3 g + k
  uint32_t iss_off = 0, iss_len = 0, sub_off = 0, sub_len = 0, jti_off = 0, jti_len = 0;
  uint32_t aud_off = 0, aud_len = 0, aud_n = 0;
  uint32_t present = 0;
};
struct NoExtract {};

// What the selecting form (claims_select) keeps beside Extract's: which of the
// caller's names the depth-1 key read so far can still be, the slot of the
// member whose value comes next, and per slot where that value lies.  The slot
// arrays are only ever touched by constant-trip loops over all eight slots
// (selects on `slot == k`), so they stay registers like the scalars.
struct SelState {
  uint32_t kcand = 0;               // bit k: the depth-1 key so far is a prefix of name k
  uint32_t ksel = 0;                // slot + 1 of the depth-1 member being read; 0: not selected
  uint32_t hi = 0;                  // the string value being read holds a byte >= 0x80
  uint32_t stype = 0;               // jg_sel_type per slot, four bits each
  uint32_t voff = 0, vtype = 0;     // the selected value that is open: where it began, its jg_sel_type
  uint32_t ev = 0, eva = 0;         // this byte ends it (1; 2: as STRING_RAW) in front of eva
  uint32_t soff[JG_MAX_SELECT] = {}, slen[JG_MAX_SELECT] = {};
};
struct ExtractSelect : Extract, SelState {};

// What the path-selecting form (claims_paths_each) keeps beside those.  Selected
// values nest here (a path may be a prefix of another), so the slot of the
// member being read is kept per depth, and a slot is latched in two steps: its
// offset and type when the value begins, its length when it ends.  kcand and
// desc hold path k at bit 2k, as Paths::ge does.
struct PathState {
  uint32_t md = 0;                  // two bits per path: j = components 1..j matched, their objects still open
  uint32_t desc = 0;                // paths whose next component is the key just read: they descend if its value is an object
  uint32_t kselv = 0;               // four bits per depth 1..4: slot + 1 of that depth's member being read
  uint32_t bv = 0;                  // this byte begins the values of these slots (bit 2k) at voff with type vtype
};
struct ExtractPath : Extract, SelState, PathState {};

// What the matching form (claims_match_each) keeps: the path matcher's state
// without any record (no span is latched, so no decoded position either), and
// the predicates.  mcand is `cand` for the predicates' values: bit k means value k
// still equals the string read so far (EQUALS, HAS_ELEMENT: at ScanT::pos) or
// its current word (HAS_WORD: at wpos).  One open string and one open array are
// enough: a path never descends into an array, so no key inside the open one
// selects anything until it closes, and an object that a shorter path selects
// around the open value can only carry PRESENT, which is decided when it begins.
struct MatchState {
  uint32_t kcand = 0, md = 0, desc = 0, kselv = 0;    // as SelState's and PathState's
  uint32_t mcand = 0;               // predicates whose value the open string, or its current word, can still be
  uint32_t mword = 0;               // the HAS_WORD predicates of the open string: a space arms them again
  uint32_t wpos = 0;                // the position inside the current word
  uint32_t marr = 0, medepth = 0;   // slot + 1 of the selected array that is open; the depth of its direct elements
  uint32_t res = 0;                 // the predicates that hold on what was read so far
};

// What the matching form with operands (claims_match_args) keeps beside
// MatchState's.  An open string can be compared with at most one operand per
// column (two predicates of one path, op and column are refused), so a window of
// four operand bytes per column is enough; like SelState's slot arrays it is only
// touched by constant-trip loops over all columns (selects on `col == c`).
struct MatchArgsState : MatchState {
  uint32_t alen = 0;                // the lane's string operands' lengths, a byte per column
  uint32_t nump = 0;                // the numeric predicates of the member whose value is being read
  uint32_t win[JG_MAX_ARGS] = {};   // per column: bytes [pos & ~3, (pos & ~3) + 4) of the lane's operand
};

// What the matching form with sets (claims_match_set) keeps beside
// MatchArgsState's: the decoded position of the byte being read (as Extract's),
// the set predicates the open string has armed, where that string's first byte
// lies, and its running hash: one for every set of the call.
struct MatchSetState : MatchArgsState {
  uint32_t dpos = 0;
  uint32_t sarm = 0;                // the IN_SET / ELEMENT_IN_SET predicates of the open string
  uint32_t sstart = 0;              // the decoded position of its first byte
  uint32_t sh = 0;                  // the hash state of the string so far (claim_set.hpp set_hash_step)
};

// The scan's compile-time modes: the verdict alone, with the jg_claims record,
// with the record and the caller's selected members (jg_selected) by name or by
// path, with the caller's predicates on members reached by path, and with
// predicates that also take an operand per token or test a number, and with
// predicates that also ask a resident set
constexpr int kVerdict = 0, kExtract = 1, kSelect = 2, kPath = 3, kMatch = 4, kMatchArgs = 5, kMatchSet = 6;
// what a mode keeps: the jg_claims record, the jg_selected record, the path matcher, the predicates
template <int M> constexpr bool kRec = M >= kExtract && M <= kPath;
template <int M> constexpr bool kSel = M >= kSelect && M <= kPath;
template <int M> constexpr bool kWalk = M == kPath || M == kMatch || M == kMatchArgs || M == kMatchSet;
template <int M> constexpr bool kPred = M == kMatch || M == kMatchArgs || M == kMatchSet;
template <int M> constexpr bool kArgs = M == kMatchArgs || M == kMatchSet;      // operands of the token's own, numeric tests

template <int M>
struct ScanT : std::conditional_t<M == kMatchSet, MatchSetState, std::conditional_t<M == kMatchArgs, MatchArgsState,
                                  std::conditional_t<M == kMatch, MatchState, std::conditional_t<M == kPath, ExtractPath,
                                  std::conditional_t<M == kSelect, ExtractSelect,
                                  std::conditional_t<M == kExtract, Extract, NoExtract>>>>>> {
  uint32_t st = ST_START;
  uint32_t depth = 0, stk = 0;      // open containers; bit d: container d+1 is an object
  uint32_t field = F_NONE;          // the top-level member whose value comes next
  uint32_t seen = 0;                // registered fields named so far
  uint32_t bad = 0;                 // not provable: the host decides
  uint32_t is_key = 0, ascii_only = 0, klen = 0, kw = 0;
  uint32_t cand = 0, pos = 0, cmpf = F_NONE;   // expected strings still equal to the value so far
  uint32_t aud_arr = 0;             // inside the aud member's array
  uint32_t nlen = 0, ndig = 0, neg = 0, isdate = 0;
  uint64_t val = 0;
  uint32_t lit = 0;                 // bytes a literal still owes, low byte first
  uint32_t str_ok = 0;              // bit f: the iss/sub/jti value equals the expected string
  uint32_t aud_found = 0;
  int64_t exp = 0, nbf = 0, iat = 0;
};
using Scan = ScanT<kVerdict>;

JG_CL_HD bool is_ws(uint32_t c) { return c == 0x20u || c == 0x09u || c == 0x0au || c == 0x0du; }
JG_CL_HD bool is_digit(uint32_t c) { return c - 0x30u < 10u; }

// claims_select: the value of the selected depth-1 member (slot ksel - 1) begins
// at decoded position `off` with jg_sel_type `type` (one such value is open at
// a time: two scalars) ...
// In a path scan the member is the one its depth's key selected, and the begin
// is an event of its own for sel_commit: an outer selected object stays open
// while an inner member is read, so nothing about it may live in these scalars.
template <int M>
JG_CL_HD uint32_t path_slot(const ScanT<M>& s) {      // slot + 1 of the member being read at this depth
  return s.depth - 1u < 4u ? (s.kselv >> (4u * (s.depth - 1u))) & 0xfu : 0u;
}
template <int M>
JG_CL_HD void sel_begin(ScanT<M>& s, uint32_t off, uint32_t type) {
  if constexpr (M == kPath) {
    const uint32_t slot = path_slot(s);
    s.bv = slot ? 1u << (2u * (slot - 1u)) : 0u;
    s.voff = off;
    s.vtype = type;
    return;
  }
  if (s.depth != 1u || !s.ksel) return;
  s.voff = off;
  s.vtype = type;
}
// ... and ends in front of `end`.  raw: a string with a byte >= 0x80, whose span
// takes the quotes in (JG_SEL_STRING_RAW)
template <int M>
JG_CL_HD void sel_end(ScanT<M>& s, uint32_t end, uint32_t raw) {
  if constexpr (M == kPath) {
    s.ksel = path_slot(s);
    if (!s.ksel) return;
    s.kselv &= ~(0xfu << (4u * (s.depth - 1u)));      // the member is read: an array's elements at this depth have no key
    s.ev = 1u + raw;
    s.eva = end;
    return;
  }
  if (s.depth != 1u || !s.ksel) return;
  s.ev = 1u + raw;
  s.eva = end;
}
// A byte ends at most one value, so step() only notes the end and the slot is
// latched here, in one place, once per byte, with values that do not depend on
// the slot: latching at each place a value can begin or end costs the kernel 50
// registers more.  The last member of a name wins: its end overwrites the slot.
template <int M>
JG_CL_HD void sel_commit(ScanT<M>& s) {
  if constexpr (M == kPath) {
    // begin: off, -off, type; end: the length is end - off, and a raw string
    // takes its quotes in.  Adds under selects: no slot is read by index.
    if (s.bv) {
      for (uint32_t k = 0; k < JG_MAX_SELECT; ++k) {
        const bool hit = (s.bv >> (2u * k)) & 1u;
        s.soff[k] = hit ? s.voff : s.soff[k];
        s.slen[k] = hit ? 0u - s.voff : s.slen[k];
        s.stype = hit ? (s.stype & ~(0xfu << (4u * k))) | (s.vtype << (4u * k)) : s.stype;
      }
      s.bv = 0;
    }
    if (s.ev) {
      const uint32_t raw = s.ev - 1u;
      s.stype += raw << (4u * (s.ksel - 1u));                      // STRING + 1 = STRING_RAW
      for (uint32_t k = 0; k < JG_MAX_SELECT; ++k) {
        const bool hit = s.ksel == k + 1u;
        s.soff[k] = hit ? s.soff[k] - raw : s.soff[k];
        s.slen[k] = hit ? s.slen[k] + s.eva + 2u * raw : s.slen[k];
      }
      s.ev = 0;
    }
    return;
  }
  if (!s.ev) return;
  const uint32_t raw = s.ev - 1u, sh = 4u * (s.ksel - 1u);
  const uint32_t off = s.voff - raw, len = s.eva + raw - off;
  s.stype = (s.stype & ~(0xfu << sh)) | ((s.vtype + raw) << sh);    // STRING + 1 = STRING_RAW
  for (uint32_t k = 0; k < JG_MAX_SELECT; ++k) {
    const bool hit = s.ksel == k + 1u;
    s.soff[k] = hit ? off : s.soff[k];
    s.slen[k] = hit ? len : s.slen[k];
  }
  s.ev = 0;
}

template <int M>
JG_CL_HD void end_value(ScanT<M>& s) { s.st = s.depth == 0 ? (uint32_t)ST_DONE : (uint32_t)ST_AFTER; }

template <int M>
JG_CL_HD void push(ScanT<M>& s, uint32_t is_obj) {
  if (s.depth >= 32u) { s.bad = 1; return; }
  s.stk = (s.stk & ~(1u << s.depth)) | (is_obj << s.depth);
  ++s.depth;
}

template <int M>
JG_CL_HD void pop(ScanT<M>& s, uint32_t is_obj) {
  if (((s.stk >> (s.depth - 1u)) & 1u) != is_obj) { s.bad = 1; return; }
  --s.depth;
  if constexpr (kRec<M>) s.aud_len = s.depth == 1u && s.aud_arr ? s.dpos + 1u - s.aud_off : s.aud_len;   // aud's ]
  if (s.depth == 1u) s.aud_arr = 0;
  if constexpr (kWalk<M>) {
    // a matched object closed: the paths that were inside it (field == depth) are one component back
    if (s.depth - 1u < 3u) {
      const uint32_t x = s.md ^ (s.depth * 0x5555u);
      s.md -= ~(x | (x >> 1)) & 0x5555u;
    }
  }
  if constexpr (kSel<M>) sel_end(s, s.dpos + 1u, 0u);          // the selected member's ] or }
  if constexpr (kPred<M>) s.marr = s.depth < s.medepth ? 0u : s.marr;   // the selected array's ]
  end_value(s);
}

// the first byte of a value
template <int M, class EX, class PQ = Preds>
JG_CL_HD void begin_value(ScanT<M>& s, uint32_t c, const EX& E, const PQ* Q = nullptr) {
  (void)Q;
  const uint32_t f = s.depth == 1u ? s.field : (uint32_t)F_NONE;
  const uint32_t elem = s.depth == 2u && s.aud_arr;        // an element of aud's array
  const uint32_t is_str3 = f - F_ISS < 3u, is_date = f - F_EXP < 3u;
  if constexpr (kWalk<M>) {                            // only an object is descended into
    s.md += c == '{' ? s.desc : 0u;
    s.desc = 0;
  }
  if constexpr (kPred<M>) {
    // The value of the member a path ends at (its key cleared the path's predicates), or a direct
    // element of that member's open array: PRESENT holds from here; a string arms the candidates.
    const uint32_t slot = path_slot(s);
    const uint32_t el = s.marr && s.depth == s.medepth ? s.marr : 0u;
    const bool str = c == '"';
    if (slot) {
      s.kselv &= ~(0xfu << (4u * (s.depth - 1u)));     // the member is read: an array's elements at this depth have no key
      s.res |= Q->present[slot - 1u];
    }
    s.mcand = !str ? 0u : slot ? Q->str[slot - 1u] : el ? Q->elem[el - 1u] : 0u;
    s.mword = str && slot ? Q->word[slot - 1u] : 0u;
    s.wpos = 0;
    if constexpr (kArgs<M>) {
      s.nump = slot ? Q->num[slot - 1u] : 0u;          // read by end_number, if this is one
      s.res |= str && slot ? Q->isstr[slot - 1u] : 0u; // IS_STRING holds from the opening quote; "" counts
    }
    if constexpr (M == kMatchSet) {
      // the set predicates arm where mcand does; the string's hash starts over
      s.sarm = !str ? 0u : slot ? Q->sets.inset[slot - 1u] : el ? Q->sets.elemset[el - 1u] : 0u;
      if (s.sarm) {
        s.sstart = s.dpos + 1u;
        s.sh = jgset::kHashBasis;
      }
    }
    if (c == '[' && slot) {
      s.marr = slot;
      s.medepth = s.depth + 1u;
    }
  }
  if (c == '"') {
    if (is_date) s.bad = 1;
    s.st = ST_STR;
    s.is_key = 0;
    s.ascii_only = f != F_NONE || elem;
    s.pos = 0;
    s.cmpf = elem ? (uint32_t)F_AUD : f;
    s.cand = is_str3 ? (E.slen(f - 1u) ? 1u << (f - 1u) : 0u)
           : (f == F_AUD || elem) ? ((1u << E.auds()) - 1u) << 3 : 0u;
    if constexpr (kRec<M>) {
      const uint32_t in = s.dpos + 1u;                 // the first byte between the quotes
      s.iss_off = f == F_ISS ? in : s.iss_off;
      s.sub_off = f == F_SUB ? in : s.sub_off;
      s.jti_off = f == F_JTI ? in : s.jti_off;
      s.aud_off = f == F_AUD ? s.dpos : s.aud_off;
      s.aud_n = f == F_AUD ? 1u : s.aud_n + elem;
      s.present |= (is_str3 || f == F_AUD) ? 1u << f : 0u;
    }
    if constexpr (kSel<M>) {
      s.hi = 0;
      sel_begin(s, s.dpos + 1u, (uint32_t)JG_SEL_STRING);
    }
  } else if (c == '{' || c == '[') {
    const uint32_t arr = c == '[';
    if constexpr (kSel<M>) sel_begin(s, s.dpos, arr ? (uint32_t)JG_SEL_ARRAY : (uint32_t)JG_SEL_OBJECT);
    if (arr && f == F_AUD) {
      s.aud_arr = 1;
      if constexpr (kRec<M>) {
        s.aud_off = s.dpos;
        s.present |= 1u << F_AUD;
      }
    } else if (f != F_NONE || elem) s.bad = 1;
    push(s, arr ^ 1u);
    s.st = arr ? (uint32_t)ST_ARR_FIRST : (uint32_t)ST_OBJ_FIRST;
  } else if (c == 't' || c == 'f' || c == 'n') {
    // null: skipped for iss/sub/jti, absent for a date; any literal elsewhere
    if ((f != F_NONE || elem) && !(c == 'n' && (is_str3 || is_date))) s.bad = 1;
    if constexpr (kSel<M>)
      sel_begin(s, s.dpos, c == 't' ? (uint32_t)JG_SEL_TRUE : c == 'f' ? (uint32_t)JG_SEL_FALSE : (uint32_t)JG_SEL_NULL);
    s.lit = c == 't' ? 0x657572u : c == 'f' ? 0x65736c61u : 0x6c6c75u;   // "rue" / "alse" / "ull"
    s.st = ST_LIT;
  } else if (c == '-' || is_digit(c)) {
    if (!is_date && (f != F_NONE || elem)) s.bad = 1;
    if constexpr (kSel<M>) sel_begin(s, s.dpos, (uint32_t)JG_SEL_NUMBER);
    s.isdate = is_date;
    s.nlen = 1;
    s.neg = c == '-';
    s.ndig = s.neg ^ 1u;
    s.val = s.neg ? 0u : c - 0x30u;
    s.st = s.neg ? (uint32_t)ST_NUM_MINUS : c == '0' ? (uint32_t)ST_NUM_ZERO : (uint32_t)ST_NUM_INT;
  } else {
    s.bad = 1;
  }
}

// a number ended in front of the current byte
template <int M, class PQ = Preds, class AR = NoArgs>
JG_CL_HD void end_number(ScanT<M>& s, const PQ* Q = nullptr, const AR* A = nullptr) {
  (void)Q;
  (void)A;
  if (s.isdate) {
    // -?(0|[1-9][0-9]{0,14}), not -0: exact in float64 and far from any wrap
    if (s.st != ST_NUM_ZERO && s.st != ST_NUM_INT) s.bad = 1;
    if (s.ndig > 15u || (s.neg && s.val == 0)) s.bad = 1;
    const int64_t v = s.neg ? -(int64_t)s.val : (int64_t)s.val;
    // selects, not one store behind a computed address (that would put Scan in scratch)
    s.exp = s.field == F_EXP ? v : s.exp;
    s.nbf = s.field == F_NBF ? v : s.nbf;
    s.iat = s.field == F_IAT ? v : s.iat;
    if constexpr (kRec<M>) s.present |= 1u << s.field;
  }
  if constexpr (kArgs<M>) {
    // The number a path with numeric predicates reaches.  Go holds it as a float64 f and the caller
    // tests f >= float64(B) or f <= float64(B).  On the date form -?(0|[1-9][0-9]{0,14}) (-0 is 0, as
    // in float64) the integer compare below is that compare for every int64 B: |v| < 10^15 < 2^53, so f
    // is v exactly; every integer up to 2^53 is a float64 and float64() rounds monotonically, so a B
    // with |B| <= 2^53 converts exactly, and one beyond converts to a value beyond +-2^53 of B's sign,
    // which lies on the same side of v as B does.  Any other form (a fraction, 16 or 17 digits) is the
    // host's: the token is JG_CL_HOST, also when a later member replaces this one.
    if (s.nump) {
      if ((s.st != ST_NUM_ZERO && s.st != ST_NUM_INT) || s.ndig > 15u) s.bad = 1;
      const int64_t v = s.neg ? -(int64_t)s.val : (int64_t)s.val;
      uint32_t m = s.nump;
      while (m) {
        const uint32_t k = (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        const int64_t b = (Q->arg >> k) & 1u ? A->bound(Q->col[k]) : Q->bound[k];
        s.res |= ((Q->le >> k) & 1u ? v <= b : v >= b) ? 1u << k : 0u;
      }
      s.nump = 0;
    }
  }
  if constexpr (kSel<M>) sel_end(s, s.dpos, 0u);                   // dpos: the byte after the literal
  // this byte may go on to close the object around the number, itself selected by a shorter path
  if constexpr (M == kPath) sel_commit(s);
  s.st = ST_AFTER;
}

// base64url alphabet -> 6 bits, 0xff for any other byte
JG_CL_HD uint32_t sextet(uint32_t c) {
  uint32_t v = 0xffu;
  v = c - 0x41u < 26u ? c - 0x41u : v;
  v = c - 0x61u < 26u ? c - 0x61u + 26u : v;
  v = c - 0x30u < 10u ? c - 0x30u + 52u : v;
  v = c == 0x2du ? 62u : v;
  v = c == 0x5fu ? 63u : v;
  return v;
}

template <int M, class EX, class SL, class PQ = Preds, class AR = NoArgs>
JG_CL_HD void step(ScanT<M>& s, uint32_t c, const EX& E, const SL* S, const PQ* Q = nullptr, const AR* A = nullptr) {
  (void)S;
  (void)Q;
  (void)A;
  if (s.st >= ST_NUM_MINUS && s.st <= ST_NUM_FRAC) {
    const uint32_t d = is_digit(c);
    uint32_t nx = ST_AFTER;                           // ST_AFTER: the number ends here
    if (s.st == ST_NUM_MINUS) nx = d ? (c == '0' ? (uint32_t)ST_NUM_ZERO : (uint32_t)ST_NUM_INT) : 0xffu;
    else if (s.st == ST_NUM_ZERO) nx = c == '.' ? (uint32_t)ST_NUM_DOT : d ? 0xffu : (uint32_t)ST_AFTER;
    else if (s.st == ST_NUM_INT) nx = d ? (uint32_t)ST_NUM_INT : c == '.' ? (uint32_t)ST_NUM_DOT : (uint32_t)ST_AFTER;
    else if (s.st == ST_NUM_DOT) nx = d ? (uint32_t)ST_NUM_FRAC : 0xffu;
    else nx = d ? (uint32_t)ST_NUM_FRAC : (uint32_t)ST_AFTER;
    if (nx == 0xffu) { s.bad = 1; return; }
    if (nx != ST_AFTER) {
      if (++s.nlen > 17u) s.bad = 1;                  // longer: Go may fail on range
      if (nx == ST_NUM_ZERO || nx == ST_NUM_INT) {
        s.val = s.val * 10u + (c - 0x30u);            // at most 17 digits: no wrap
        ++s.ndig;
      }
      s.st = nx;
      return;
    }
    end_number(s, Q, A);                              // ... and the byte is read as what follows a value
  }
  switch (s.st) {
    case ST_STR:
      if (c == '"') {
        if (s.is_key) {
          s.st = ST_COLON;
          if (s.depth == 1u) {
            s.field = s.klen == 3u ? field_of(s.kw) : (uint32_t)F_NONE;
            if (s.field != F_NONE) {
              if ((s.seen >> s.field) & 1u) s.bad = 1;          // named twice: Go takes the last in sorted order
              s.seen |= 1u << s.field;
            }
            if constexpr (M == kSelect) {                       // the name this key is, exactly, or none
              uint32_t m = s.kcand, slot = 0;
              while (m) {
                const uint32_t k = (uint32_t)__builtin_ctz(m);
                m &= m - 1u;
                slot = S->len[k] == s.klen ? k + 1u : slot;
              }
              s.ksel = slot;
            }
          }
          if constexpr (kWalk<M>) {
            // The survivors of this length are this key.  The path that ends here selects the
            // member (equal paths are refused: at most one); a longer one descends if the value is
            // an object, and its slot is ABSENT from here on: this member replaces an earlier one.
            const uint32_t d = s.depth;
            uint32_t m = s.kcand, slot = 0, desc = 0, through = 0;
            while (m) {
              const uint32_t b = (uint32_t)__builtin_ctz(m), k = b >> 1;
              m &= m - 1u;
              const bool is = S->len[k][d - 1u] == s.klen, last = S->ncomp[k] == d;
              slot = is && last ? k + 1u : slot;
              desc |= is && !last ? 1u << b : 0u;
              if constexpr (kPred<M>) through |= is ? Q->all[k] : 0u;
            }
            (void)through;
            s.desc = desc;
            if (d - 1u < 4u) s.kselv = (s.kselv & ~(0xfu << (4u * (d - 1u)))) | (slot << (4u * (d - 1u)));
            if constexpr (M == kPath) {
              s.bv = desc;                                      // sel_commit: ABSENT, as a value of type 0 at 0
              s.voff = 0;
              s.vtype = 0;
            }
            // a match scan: the same member takes back what an earlier one of that key gave every path through it
            if constexpr (kPred<M>) s.res &= ~through;
          }
        } else {
          uint32_t m = s.cand, hit = 0;
          while (m) {
            const uint32_t k = (uint32_t)__builtin_ctz(m);
            m &= m - 1u;
            hit |= E.slen(k) == s.pos;
          }
          if (s.cmpf == F_AUD) s.aud_found |= hit;
          else if (s.cmpf != F_NONE) s.str_ok |= hit << s.cmpf;
          if constexpr (kRec<M>) {
            s.iss_len = s.cmpf == F_ISS ? s.pos : s.iss_len;
            s.sub_len = s.cmpf == F_SUB ? s.pos : s.sub_len;
            s.jti_len = s.cmpf == F_JTI ? s.pos : s.jti_len;
            s.aud_len = s.cmpf == F_AUD && !s.aud_arr ? s.dpos + 1u - s.aud_off : s.aud_len;   // aud as one string
          }
          if constexpr (kSel<M>) sel_end(s, s.dpos, s.hi);
          if constexpr (kPred<M>) {                             // the survivors of this length are the string, or its last word
            uint32_t mm = s.mcand;
            while (mm) {
              const uint32_t k = (uint32_t)__builtin_ctz(mm);
              mm &= mm - 1u;
              uint32_t l = Q->len[k];
              if constexpr (kArgs<M>) l = (Q->arg >> k) & 1u ? (s.alen >> (8u * Q->col[k])) & 0xffu : l;
              s.res |= l == ((s.mword >> k) & 1u ? s.wpos : s.pos) ? 1u << k : 0u;
            }
            s.mcand = 0;
            s.mword = 0;
          }
          if constexpr (M == kMatchSet) {
            // The armed set predicates: the string's hash, finalised with the seed of the predicate's set, is looked up in
            // that set's table, and a slot of this hash and length is confirmed against the string
            // itself, decoded again from the payload: byte o is byte o % 3 of group o / 3, a group
            // the scan has read already (sextets valid, inside the segment's seven bytes of slack).
            uint32_t mm = s.sarm;
            if (mm) {
              uint32_t cg = 0xffffffffu, trip = 0;
              const uint32_t start = s.sstart;
              auto cmp = [&](uint32_t i) -> uint32_t {
                const uint32_t o = start + i, g = o / 3u;
                if (g != cg) {
                  const uint32_t w = A->peek(g);
                  cg = g;
                  trip = ((sextet(w & 0xffu) & 63u) << 18) | ((sextet((w >> 8) & 0xffu) & 63u) << 12) |
                         ((sextet((w >> 16) & 0xffu) & 63u) << 6) | (sextet(w >> 24) & 63u);
                }
                return (trip >> (16u - 8u * (o - 3u * g))) & 0xffu;
              };
              while (mm) {
                const uint32_t k = (uint32_t)__builtin_ctz(mm);
                mm &= mm - 1u;
                const uint32_t x = Q->sets.set[k];
                const SetHeader& H = Q->sets.h[x];
                const jgset::View V{(const jgset::Slot*)(uintptr_t)H.slots, (const uint32_t*)(uintptr_t)H.pool,
                                    H.mask, H.maxprobe, H.seed, H.n};
                s.res |= jgset::set_probe(V, jgset::set_hash_final(s.sh, H.seed), s.pos, cmp) ? 1u << k : 0u;
              }
              s.sarm = 0;
            }
          }
          end_value(s);
        }
      } else {
        if (c < 0x20u || c == '\\') s.bad = 1;
        if (c >= 0x80u && s.ascii_only) s.bad = 1;
        if constexpr (kSel<M>) s.hi |= c >= 0x80u;
        if (s.is_key) {
          if constexpr (M == kSelect) {                         // names still equal to the key so far
            uint32_t m = s.kcand;
            while (m) {
              const uint32_t k = (uint32_t)__builtin_ctz(m);
              m &= m - 1u;
              if (!(s.klen < S->len[k] && S->bytes[S->off[k] + s.klen] == c)) s.kcand &= ~(1u << k);
            }
          }
          if constexpr (kWalk<M>) {                             // paths whose component at this depth still equals the key so far
            uint32_t m = s.kcand;
            while (m) {
              const uint32_t b = (uint32_t)__builtin_ctz(m), k = b >> 1;
              m &= m - 1u;
              if (!(s.klen < S->len[k][s.depth - 1u] && S->pool[S->off[k][s.depth - 1u] + s.klen] == c))
                s.kcand &= ~(1u << b);
            }
          }
          if (s.klen < 3u) s.kw = (s.kw << 8) | (c - 0x61u < 26u ? c - 0x20u : c);
          ++s.klen;
        }
        if constexpr (kPred<M>) {
          // Predicates whose value still equals the string (at pos) or its current word (at wpos).  A
          // space ends a word -- the word candidates of its length hold -- and arms them all again.
          const uint32_t sp = c == 0x20u ? s.mword : 0u;
          uint32_t mm = s.mcand;
          while (mm) {
            const uint32_t k = (uint32_t)__builtin_ctz(mm);
            mm &= mm - 1u;
            if constexpr (kArgs<M>) {
              // An operand of the lane's own: its length from alen, its byte from the column's window,
              // which is filled from global memory at every fourth byte while the candidate survives.
              if ((Q->arg >> k) & 1u) {
                const uint32_t col = Q->col[k], at = s.pos, l = (s.alen >> (8u * col)) & 0xffu;
                uint32_t w = 0;
                if (at < l && (at & 3u) == 0u) {
                  w = A->word(col, at);
                  for (uint32_t x = 0; x < JG_MAX_ARGS; ++x) s.win[x] = x == col ? w : s.win[x];
                } else {
                  for (uint32_t x = 0; x < JG_MAX_ARGS; ++x) w = x == col ? s.win[x] : w;
                }
                if (!(at < l && ((w >> (8u * (at & 3u))) & 0xffu) == c)) s.mcand &= ~(1u << k);
                continue;
              }
            }
            const uint32_t at = (s.mword >> k) & 1u ? s.wpos : s.pos, l = Q->len[k];
            s.res |= l == at ? sp & (1u << k) : 0u;
            if (!(at < l && Q->pool[Q->off[k] + at] == c)) s.mcand &= ~(1u << k);
          }
          s.mcand |= sp;
          s.wpos = sp ? 0u : s.wpos + 1u;
        }
        if constexpr (M == kMatchSet) {
          s.sh = s.sarm ? jgset::set_hash_step(s.sh, c) : s.sh;
        }
        uint32_t m = s.cand;
        while (m) {
          const uint32_t k = (uint32_t)__builtin_ctz(m);
          m &= m - 1u;
          if (!(s.pos < E.slen(k) && E.sbyte(k, s.pos) == c)) s.cand &= ~(1u << k);
        }
        ++s.pos;
      }
      break;
    case ST_LIT:
      if (c != (s.lit & 0xffu)) s.bad = 1;
      s.lit >>= 8;
      if (s.lit == 0) {
        if constexpr (kSel<M>) sel_end(s, s.dpos + 1u, 0u);
        end_value(s);
      }
      break;
    case ST_START:
      if (c == '{') { push(s, 1u); s.st = ST_OBJ_FIRST; }
      else if (!is_ws(c)) s.bad = 1;                   // null, an array, a scalar: the host's business
      break;
    case ST_VALUE:
      if (!is_ws(c)) begin_value(s, c, E, Q);
      break;
    case ST_ARR_FIRST:
      if (c == ']') pop(s, 0u);
      else if (!is_ws(c)) begin_value(s, c, E, Q);
      break;
    case ST_OBJ_FIRST:
    case ST_OBJ_KEY:
      if (c == '"') {
        s.st = ST_STR;
        s.is_key = 1;
        s.ascii_only = s.depth == 1u;
        s.klen = 0;
        s.kw = 0;
        s.cand = 0;
        if constexpr (M == kSelect) s.kcand = s.depth == 1u ? (1u << S->n) - 1u : 0u;
        if constexpr (kWalk<M>) {                        // the paths that are matched down to the object this key is in
          const uint32_t x = s.md ^ ((s.depth - 1u) * 0x5555u);
          s.kcand = s.depth - 1u < 4u ? ~(x | (x >> 1)) & S->ge[s.depth - 1u] : 0u;
        }
      } else if (c == '}' && s.st == ST_OBJ_FIRST) {
        pop(s, 1u);
      } else if (!is_ws(c)) {
        s.bad = 1;
      }
      break;
    case ST_COLON:
      if (c == ':') s.st = ST_VALUE;
      else if (!is_ws(c)) s.bad = 1;
      break;
    case ST_AFTER:
      if (c == ',') {
        if (s.depth == 1u) s.field = F_NONE;
        s.st = ((s.stk >> (s.depth - 1u)) & 1u) ? (uint32_t)ST_OBJ_KEY : (uint32_t)ST_VALUE;
      } else if (c == '}') {
        pop(s, 1u);
      } else if (c == ']') {
        pop(s, 0u);
      } else if (!is_ws(c)) {
        s.bad = 1;
      }
      break;
    default:                                            // ST_DONE: whitespace only
      if (!is_ws(c)) s.bad = 1;
      break;
  }
}

// jwt/jwt.go:117-199 on the scanned fields, in Validate's order
template <int M, class EX>
JG_CL_HD uint8_t verdict(const ScanT<M>& s, const EX& E) {
  int64_t iat = s.iat, exp = s.exp, nbf = s.nbf;
  if (iat == 0 && exp == 0 && nbf == 0) return JG_CL_NO_TIME;
  if (exp == 0) exp = (nbf > iat ? nbf : iat) + E.exp_leeway();
  if (nbf == 0) nbf = iat != 0 ? iat : exp - E.nbf_leeway();
  if (E.slen(0u) && !((s.str_ok >> F_ISS) & 1u)) return JG_CL_ISS;
  if (E.slen(1u) && !((s.str_ok >> F_SUB) & 1u)) return JG_CL_SUB;
  if (E.slen(2u) && !((s.str_ok >> F_JTI) & 1u)) return JG_CL_JTI;
  if (E.auds() && !s.aud_found) return JG_CL_AUD;
  // time.Unix(x, 0) is (x + unixToInternal, 0): Before / After on (sec, nsec)
  if (E.hi() < nbf + kUnixToInternal) return JG_CL_NBF;
  const int64_t e = exp + kUnixToInternal;
  if (E.lo() > e || (E.lo() == e && E.lons() > 0)) return JG_CL_EXP;
  if (E.hi() < iat + kUnixToInternal) return JG_CL_IAT;
  return JG_CL_OK;
}

// The scan of one segment: claims_decide's code and, with X, the record.  The
// state is a local of this function (handing it in by reference costs the
// verdict-only kernel a third of its registers again).
template <int M, class Src, class EX, class SL = Select, class PQ = Preds, class AR = NoArgs>
JG_CL_HD uint8_t scan_segment(Src& src, uint32_t len, const EX& E, jg_claims* out, const SL* S = nullptr,
                              jg_selected* sel = nullptr, const PQ* Q = nullptr, uint32_t* match = nullptr,
                              const AR* A = nullptr) {
  (void)A;
  if constexpr (kPred<M>) *match = 0;                              // JG_CL_HOST: no bit
  if constexpr (kRec<M>) *out = jg_claims{};                       // JG_CL_HOST: every byte zero
  if constexpr (kSel<M>) *sel = jg_selected{};
  if ((len & 3u) == 1u) return JG_CL_HOST;
  ScanT<M> s;
  if constexpr (kArgs<M>) {
    for (uint32_t x = 0; x < JG_MAX_ARGS; ++x) s.alen |= x < A->nstr() ? A->slen(x) << (8u * x) : 0u;
  }
  const uint32_t groups = (len + 3u) >> 2;
  for (uint32_t g = 0; g < groups && !s.bad; ++g) {
    const uint32_t w = src.word(g);
    const uint32_t rem = len - 4u * g;                 // characters of this group: 2, 3 or >= 4
    const uint32_t a = sextet(w & 0xffu), b = sextet((w >> 8) & 0xffu);
    const uint32_t c = rem > 2u ? sextet((w >> 16) & 0xffu) : 0u, d = rem > 3u ? sextet(w >> 24) : 0u;
    if ((a | b | c | d) > 63u) return JG_CL_HOST;
    uint32_t trip = (a << 18) | (b << 12) | (c << 6) | d;
    const uint32_t nb = rem > 3u ? 3u : rem - 1u;
    // Go's strict decoding: the bits the last group does not use are zero
    if (nb < 3u && (trip & (nb == 1u ? 0xffffu : 0xffu))) return JG_CL_HOST;
    for (uint32_t k = 0; k < nb; ++k) {
      if constexpr (kRec<M> || M == kMatchSet) s.dpos = 3u * g + k;
      step(s, (trip >> 16) & 0xffu, E, S, Q, A);
      if constexpr (kSel<M>) sel_commit(s);
      trip <<= 8;
    }
  }
  if (s.bad || s.st != ST_DONE) return JG_CL_HOST;
  if constexpr (kRec<M>) {
    out->exp = s.exp;
    out->nbf = s.nbf;
    out->iat = s.iat;
    out->iss_off = s.iss_off;
    out->iss_len = s.iss_len;
    out->sub_off = s.sub_off;
    out->sub_len = s.sub_len;
    out->jti_off = s.jti_off;
    out->jti_len = s.jti_len;
    out->aud_off = s.aud_off;
    out->aud_len = s.aud_len;
    out->aud_n = s.aud_n;
    out->present = s.present;
  }
  if constexpr (kSel<M>) {
    for (uint32_t k = 0; k < JG_MAX_SELECT; ++k) {
      sel->off[k] = s.soff[k];
      sel->len[k] = s.slen[k];
      sel->type[k] = (uint8_t)((s.stype >> (4u * k)) & 0xfu);
    }
  }
  if constexpr (kPred<M>) *match = s.res;
  return verdict(s, E);
}

template <class Src>
JG_CL_HD uint8_t claims_decide(Src& src, uint32_t len, const Expect& E) {
  return scan_segment<kVerdict>(src, len, E, nullptr);
}

// claims_decide's code for the same input, always, and the registered claims
// (include/jg.h jg_claims): filled for every code other than JG_CL_HOST, all
// zero for JG_CL_HOST.  The scan's rules make the spans the Go strings: a
// registered value with an escape or a byte >= 0x80, or named twice, is HOST.
template <class Src>
JG_CL_HD uint8_t claims_extract(Src& src, uint32_t len, const Expect& E, jg_claims* out) {
  return scan_segment<kExtract>(src, len, E, out);
}

// claims_extract's code and record for the same input, always, and the
// top-level members the caller named (include/jg.h jg_selected): slot k
// describes the last depth-1 member whose key is name k byte for byte.  Filled
// for every code other than JG_CL_HOST, all zero for JG_CL_HOST.
template <class Src>
JG_CL_HD uint8_t claims_select(Src& src, uint32_t len, const Expect& E, const Select& S, jg_claims* out,
                               jg_selected* sel) {
  return scan_segment<kSelect>(src, len, E, out, &S, sel);
}

// The three functions above against profile p (< T.n) of a table: for every
// segment the code and the records that the single-Expect function returns for
// resolve(x[p]), byte for byte.  The same scan_segment, with the expected side
// read through ProfileRef.
template <class Src>
JG_CL_HD uint8_t claims_decide_each(Src& src, uint32_t len, const Profiles& T, uint32_t p) {
  const ProfileRef E{T, p};
  return scan_segment<kVerdict>(src, len, E, nullptr);
}
template <class Src>
JG_CL_HD uint8_t claims_extract_each(Src& src, uint32_t len, const Profiles& T, uint32_t p, jg_claims* out) {
  const ProfileRef E{T, p};
  return scan_segment<kExtract>(src, len, E, out);
}
template <class Src>
JG_CL_HD uint8_t claims_select_each(Src& src, uint32_t len, const Profiles& T, uint32_t p, const Select& S,
                                    jg_claims* out, jg_selected* sel) {
  const ProfileRef E{T, p};
  return scan_segment<kSelect>(src, len, E, out, &S, sel);
}

// claims_extract_each's code and record for the same input, always, and the
// members the caller's paths reach (include/jg.h jg_claims_paths): slot k
// describes, as claims_select describes a top-level member, the value found by
// taking, component by component, the last member of that name in the object
// reached so far; ABSENT where a component is missing or what it names is not an
// object.  Filled for every code other than JG_CL_HOST, all zero for JG_CL_HOST.
template <class Src>
JG_CL_HD uint8_t claims_paths_each(Src& src, uint32_t len, const Profiles& T, uint32_t p, const Paths& P,
                                   jg_claims* out, jg_selected* sel) {
  const ProfileRef E{T, p};
  return scan_segment<kPath>(src, len, E, out, &P, sel);
}

// claims_decide_each's code for the same input, always, and the predicates that
// hold (include/jg.h jg_claims_match): bit k of *match is set when predicate k
// of Q holds on the value claims_paths_each's walk reaches along its path.
// Filled for every code other than JG_CL_HOST, 0 for JG_CL_HOST.
template <class Src>
JG_CL_HD uint8_t claims_match_each(Src& src, uint32_t len, const Profiles& T, uint32_t p, const Paths& P,
                                   const Preds& Q, uint32_t* match) {
  const ProfileRef E{T, p};
  return scan_segment<kMatch>(src, len, E, nullptr, &P, nullptr, &Q, match);
}

// claims_match_each's code and mask for a list of its ops, always, and the five
// ops of jg_claims_match_args (include/jg.h): A is the token's own operands --
//   uint32_t nstr()                        the string columns
//   uint32_t slen(uint32_t c)              the length of the operand in column c
//   uint32_t word(uint32_t c, uint32_t p)  its bytes [p, p + 4), little-endian, for p < slen(c), p % 4 == 0
//   int64_t bound(uint32_t c)              the number in column c
// The one difference in the code: JG_CL_HOST, mask 0, when the full path of a
// numeric predicate reaches a number literal outside -?(0|[1-9][0-9]{0,14}).
template <class Src, class AR>
JG_CL_HD uint8_t claims_match_args(Src& src, uint32_t len, const Profiles& T, uint32_t p, const Paths& P,
                                   const ArgPreds& Q, const AR& A, uint32_t* match) {
  const ProfileRef E{T, p};
  return scan_segment<kMatchArgs>(src, len, E, nullptr, &P, nullptr, &Q, match, &A);
}

// claims_match_args' code and mask for a list of its ops, always (IS_STRING
// included), and the two ops of jg_claims_match_set (include/jg.h): A is
// claims_match_args' and also gives the segment again --
//   uint32_t peek(uint32_t g)              Src::word(g), for any group the scan has read, in any order
// No code changes and none becomes JG_CL_HOST because of the two ops.
template <class Src, class AR>
JG_CL_HD uint8_t claims_match_set(Src& src, uint32_t len, const Profiles& T, uint32_t p, const Paths& P,
                                  const SetArgPreds& Q, const AR& A, uint32_t* match) {
  const ProfileRef E{T, p};
  return scan_segment<kMatchSet>(src, len, E, nullptr, &P, nullptr, &Q, match, &A);
}

}  // namespace jgclaims

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// One launch of the scan: code_out[i] = the jg_claim_code of jobs[i].  Every
// pointer is a device one.  What the struct holds picks the kernel:
//   expect           one Expected for the call; every job's flags are 0
//   table            a profile per job: jobs[i].flags (< table->n) names job i's
//   neither select nor paths: vals_out ? k_claims_extract[_each] : k_claims_scan[_each]
//   select, sel_out  k_claims_select[_each]: and sel_out[i] = the members `select` names (with vals_out)
//   paths, sel_out   k_claims_paths_each: `paths` in the place of the names (with table and vals_out)
//   paths, preds, match_out   k_claims_match_each: match_out[i] = the predicates that hold (with table; no record)
//   paths, apreds, match_out  k_claims_match_args: the same with apreds in the place of preds, and job i's operands:
//                             arg_str[i * nstr + c] (a span of arg_bytes, which has ARENA_SLACK behind it) and
//                             arg_num[i * nnum + c]
//   paths, spreds, match_out  k_claims_match_set: the same with spreds in the place of apreds (its set headers hold
//                             device addresses); picked only for a list that names a set op
struct ClaimsLaunch {
  const uint8_t* arena = nullptr;
  const jg_cjob* jobs = nullptr;
  int64_t n = 0;
  const jgclaims::Expect* expect = nullptr;
  const jgclaims::Profiles* table = nullptr;
  const jgclaims::Select* select = nullptr;
  const jgclaims::Paths* paths = nullptr;
  const jgclaims::Preds* preds = nullptr;
  const jgclaims::ArgPreds* apreds = nullptr;
  const jgclaims::SetArgPreds* spreds = nullptr;
  const uint8_t* arg_bytes = nullptr;
  const jg_sarg* arg_str = nullptr;
  const int64_t* arg_num = nullptr;
  uint32_t nstr = 0, nnum = 0;
  uint8_t* code_out = nullptr;
  jg_claims* vals_out = nullptr;
  jg_selected* sel_out = nullptr;
  uint32_t* match_out = nullptr;
};
void launch_claims(const ClaimsLaunch& c, hipStream_t s);
#endif
