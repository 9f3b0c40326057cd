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
// time (ScanT<true>): the same code, plus a jg_claims record of the registered
// claims -- the dates as numbers, iss / sub / jti / aud as byte spans into the
// decoded payload.  ScanT<false> is the verdict-only scan, unchanged.
#pragma once
#include <cstdint>
#include <type_traits>

#include "../../../include/jg.h"

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

// Fills *E from the ABI's jg_expect.  False: more than JG_MAX_AUD audiences,
// strings over JG_EXPECT_MAX_BYTES in total (or one over 65535), a bad now.
inline bool resolve(const jg_expect& x, Expect* E) {
  if (x.naud > JG_MAX_AUD || x.now_nsec >= (uint32_t)kNsPerSec) return false;
  uint64_t total = (uint64_t)x.iss_len + x.sub_len + x.jti_len;
  for (uint32_t k = 0; k < x.naud; ++k) total += x.aud_len[k];
  if (total > JG_EXPECT_MAX_BYTES || (total && !x.strs)) return false;
  int32_t hi_ns;
  time_add(x.now_sec + kUnixToInternal, x.now_nsec, x.skew_ns, &E->hi_sec, &hi_ns);
  time_add(x.now_sec + kUnixToInternal, x.now_nsec, -x.skew_ns, &E->lo_sec, &E->lo_ns);
  E->naud = x.naud;
  E->exp_leeway_s = x.exp_leeway_s;
  E->nbf_leeway_s = x.nbf_leeway_s;
  uint32_t o = 0;
  for (int k = 0; k < kStrings; ++k) {
    const uint32_t l = k == 0 ? x.iss_len : k == 1 ? x.sub_len : k == 2 ? x.jti_len
                       : (uint32_t)(k - 3) < x.naud ? x.aud_len[k - 3] : 0u;
    E->len[k] = (uint16_t)l;
    E->off[k] = (uint16_t)o;
    for (uint32_t b = 0; b < l; ++b) E->bytes[o + b] = x.strs[o + b];
    o += l;
  }
  for (uint32_t b = o; b < JG_EXPECT_MAX_BYTES; ++b) E->bytes[b] = 0;
  return true;
}

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

// X: also record the claim values (Extract); X = false is the verdict-only scan
template <bool X>
struct ScanT : std::conditional_t<X, Extract, NoExtract> {
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
using Scan = ScanT<false>;

JG_CL_HD bool is_ws(uint32_t c) { return c == 0x20u || c == 0x09u || c == 0x0au || c == 0x0du; }
JG_CL_HD bool is_digit(uint32_t c) { return c - 0x30u < 10u; }

template <bool X>
JG_CL_HD void end_value(ScanT<X>& s) { s.st = s.depth == 0 ? (uint32_t)ST_DONE : (uint32_t)ST_AFTER; }

template <bool X>
JG_CL_HD void push(ScanT<X>& s, uint32_t is_obj) {
  if (s.depth >= 32u) { s.bad = 1; return; }
  s.stk = (s.stk & ~(1u << s.depth)) | (is_obj << s.depth);
  ++s.depth;
}

template <bool X>
JG_CL_HD void pop(ScanT<X>& s, uint32_t is_obj) {
  if (((s.stk >> (s.depth - 1u)) & 1u) != is_obj) { s.bad = 1; return; }
  --s.depth;
  if constexpr (X) s.aud_len = s.depth == 1u && s.aud_arr ? s.dpos + 1u - s.aud_off : s.aud_len;   // aud's ]
  if (s.depth == 1u) s.aud_arr = 0;
  end_value(s);
}

// the first byte of a value
template <bool X>
JG_CL_HD void begin_value(ScanT<X>& s, uint32_t c, const Expect& E) {
  const uint32_t f = s.depth == 1u ? s.field : (uint32_t)F_NONE;
  const uint32_t elem = s.depth == 2u && s.aud_arr;        // an element of aud's array
  const uint32_t is_str3 = f - F_ISS < 3u, is_date = f - F_EXP < 3u;
  if (c == '"') {
    if (is_date) s.bad = 1;
    s.st = ST_STR;
    s.is_key = 0;
    s.ascii_only = f != F_NONE || elem;
    s.pos = 0;
    s.cmpf = elem ? (uint32_t)F_AUD : f;
    s.cand = is_str3 ? (E.len[f - 1u] ? 1u << (f - 1u) : 0u)
           : (f == F_AUD || elem) ? ((1u << E.naud) - 1u) << 3 : 0u;
    if constexpr (X) {
      const uint32_t in = s.dpos + 1u;                 // the first byte between the quotes
      s.iss_off = f == F_ISS ? in : s.iss_off;
      s.sub_off = f == F_SUB ? in : s.sub_off;
      s.jti_off = f == F_JTI ? in : s.jti_off;
      s.aud_off = f == F_AUD ? s.dpos : s.aud_off;
      s.aud_n = f == F_AUD ? 1u : s.aud_n + elem;
      s.present |= (is_str3 || f == F_AUD) ? 1u << f : 0u;
    }
  } else if (c == '{' || c == '[') {
    const uint32_t arr = c == '[';
    if (arr && f == F_AUD) {
      s.aud_arr = 1;
      if constexpr (X) {
        s.aud_off = s.dpos;
        s.present |= 1u << F_AUD;
      }
    } else if (f != F_NONE || elem) s.bad = 1;
    push(s, arr ^ 1u);
    s.st = arr ? (uint32_t)ST_ARR_FIRST : (uint32_t)ST_OBJ_FIRST;
  } else if (c == 't' || c == 'f' || c == 'n') {
    // null: skipped for iss/sub/jti, absent for a date; any literal elsewhere
    if ((f != F_NONE || elem) && !(c == 'n' && (is_str3 || is_date))) s.bad = 1;
    s.lit = c == 't' ? 0x657572u : c == 'f' ? 0x65736c61u : 0x6c6c75u;   // "rue" / "alse" / "ull"
    s.st = ST_LIT;
  } else if (c == '-' || is_digit(c)) {
    if (!is_date && (f != F_NONE || elem)) s.bad = 1;
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
template <bool X>
JG_CL_HD void end_number(ScanT<X>& s) {
  if (s.isdate) {
    // -?(0|[1-9][0-9]{0,14}), not -0: exact in float64 and far from any wrap
    if (s.st != ST_NUM_ZERO && s.st != ST_NUM_INT) s.bad = 1;
    if (s.ndig > 15u || (s.neg && s.val == 0)) s.bad = 1;
    const int64_t v = s.neg ? -(int64_t)s.val : (int64_t)s.val;
    // selects, not one store behind a computed address (that would put Scan in scratch)
    s.exp = s.field == F_EXP ? v : s.exp;
    s.nbf = s.field == F_NBF ? v : s.nbf;
    s.iat = s.field == F_IAT ? v : s.iat;
    if constexpr (X) s.present |= 1u << s.field;
  }
  s.st = ST_AFTER;
}

template <bool X>
JG_CL_HD void step(ScanT<X>& s, uint32_t c, const Expect& E) {
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
    end_number(s);                                    // ... and the byte is read as what follows a value
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
          }
        } else {
          uint32_t m = s.cand, hit = 0;
          while (m) {
            const uint32_t k = (uint32_t)__builtin_ctz(m);
            m &= m - 1u;
            hit |= E.len[k] == s.pos;
          }
          if (s.cmpf == F_AUD) s.aud_found |= hit;
          else if (s.cmpf != F_NONE) s.str_ok |= hit << s.cmpf;
          if constexpr (X) {
            s.iss_len = s.cmpf == F_ISS ? s.pos : s.iss_len;
            s.sub_len = s.cmpf == F_SUB ? s.pos : s.sub_len;
            s.jti_len = s.cmpf == F_JTI ? s.pos : s.jti_len;
            s.aud_len = s.cmpf == F_AUD && !s.aud_arr ? s.dpos + 1u - s.aud_off : s.aud_len;   // aud as one string
          }
          end_value(s);
        }
      } else {
        if (c < 0x20u || c == '\\') s.bad = 1;
        if (c >= 0x80u && s.ascii_only) s.bad = 1;
        if (s.is_key) {
          if (s.klen < 3u) s.kw = (s.kw << 8) | (c - 0x61u < 26u ? c - 0x20u : c);
          ++s.klen;
        }
        uint32_t m = s.cand;
        while (m) {
          const uint32_t k = (uint32_t)__builtin_ctz(m);
          m &= m - 1u;
          if (!(s.pos < E.len[k] && E.bytes[E.off[k] + s.pos] == c)) s.cand &= ~(1u << k);
        }
        ++s.pos;
      }
      break;
    case ST_LIT:
      if (c != (s.lit & 0xffu)) s.bad = 1;
      s.lit >>= 8;
      if (s.lit == 0) end_value(s);
      break;
    case ST_START:
      if (c == '{') { push(s, 1u); s.st = ST_OBJ_FIRST; }
      else if (!is_ws(c)) s.bad = 1;                   // null, an array, a scalar: the host's business
      break;
    case ST_VALUE:
      if (!is_ws(c)) begin_value(s, c, E);
      break;
    case ST_ARR_FIRST:
      if (c == ']') pop(s, 0u);
      else if (!is_ws(c)) begin_value(s, c, E);
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

// jwt/jwt.go:117-199 on the scanned fields, in Validate's order
template <bool X>
JG_CL_HD uint8_t verdict(const ScanT<X>& s, const Expect& E) {
  int64_t iat = s.iat, exp = s.exp, nbf = s.nbf;
  if (iat == 0 && exp == 0 && nbf == 0) return JG_CL_NO_TIME;
  if (exp == 0) exp = (nbf > iat ? nbf : iat) + E.exp_leeway_s;
  if (nbf == 0) nbf = iat != 0 ? iat : exp - E.nbf_leeway_s;
  if (E.len[0] && !((s.str_ok >> F_ISS) & 1u)) return JG_CL_ISS;
  if (E.len[1] && !((s.str_ok >> F_SUB) & 1u)) return JG_CL_SUB;
  if (E.len[2] && !((s.str_ok >> F_JTI) & 1u)) return JG_CL_JTI;
  if (E.naud && !s.aud_found) return JG_CL_AUD;
  // time.Unix(x, 0) is (x + unixToInternal, 0): Before / After on (sec, nsec)
  if (E.hi_sec < nbf + kUnixToInternal) return JG_CL_NBF;
  const int64_t e = exp + kUnixToInternal;
  if (E.lo_sec > e || (E.lo_sec == e && E.lo_ns > 0)) return JG_CL_EXP;
  if (E.hi_sec < iat + kUnixToInternal) return JG_CL_IAT;
  return JG_CL_OK;
}

// The scan of one segment: claims_decide's code and, with X, the record.  The
// state is a local of this function (handing it in by reference costs the
// verdict-only kernel a third of its registers again).
template <bool X, class Src>
JG_CL_HD uint8_t scan_segment(Src& src, uint32_t len, const Expect& E, jg_claims* out) {
  if constexpr (X) *out = jg_claims{};                 // JG_CL_HOST: every byte zero
  if ((len & 3u) == 1u) return JG_CL_HOST;
  ScanT<X> s;
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
      if constexpr (X) s.dpos = 3u * g + k;
      step(s, (trip >> 16) & 0xffu, E);
      trip <<= 8;
    }
  }
  if (s.bad || s.st != ST_DONE) return JG_CL_HOST;
  if constexpr (X) {
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
  return verdict(s, E);
}

template <class Src>
JG_CL_HD uint8_t claims_decide(Src& src, uint32_t len, const Expect& E) {
  return scan_segment<false>(src, len, E, nullptr);
}

// claims_decide's code for the same input, always, and the registered claims
// (include/jg.h jg_claims): filled for every code other than JG_CL_HOST, all
// zero for JG_CL_HOST.  The scan's rules make the spans the Go strings: a
// registered value with an escape or a byte >= 0x80, or named twice, is HOST.
template <class Src>
JG_CL_HD uint8_t claims_extract(Src& src, uint32_t len, const Expect& E, jg_claims* out) {
  return scan_segment<true>(src, len, E, out);
}

}  // namespace jgclaims

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// code_out[i] = the jg_claim_code of jobs[i]; `expect` is a device jgclaims::Expect
void launch_claims_scan(const uint8_t* arena, const jg_cjob* jobs, int64_t n, const jgclaims::Expect* expect,
                        uint8_t* code_out, hipStream_t s);
// ... and vals_out[i] = its registered claims (k_claims_extract)
void launch_claims_extract(const uint8_t* arena, const jg_cjob* jobs, int64_t n, const jgclaims::Expect* expect,
                           uint8_t* code_out, jg_claims* vals_out, hipStream_t s);
#endif
