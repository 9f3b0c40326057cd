/*
 * jg.h -- C ABI of the MI355X batched JWS signature verifier (libcapjwt.so).
 *
 * This is the drop-in boundary for cap's signature-verification hot path.  A Go
 * maintainer binds it with cgo underneath a GPU-backed
 * implementation of cap's KeySet interface:
 *
 *   type KeySet interface {                                 jwt/keyset.go:27-32
 *     VerifySignature(ctx, token string) (map[string]interface{}, error)
 *   }
 *
 * Each entry point replaces one piece of the reference's per-token call stack
 *  with a batched, device-side equivalent:
 *
 *   jg_keys_load     <- key ingestion: NewStaticKeySet (jwt/keyset.go:142-150),
 *                       JWKS decode in go-oidc RemoteKeySet (jwt/keyset.go:101,120)
 *   jg_verify_batch  <- the signature arithmetic of parsedJWT.Claims(key, ...)
 *                       (jwt/keyset.go:163) / remoteJWKS.VerifySignature
 *                       (jwt/keyset.go:127): go-jose verifyPayload -> crypto/rsa
 *                       VerifyPKCS1v15 | VerifyPSS, crypto/ecdsa.Verify,
 *                       crypto/ed25519.Verify, for MANY (token, key) pairs at once
 *
 * Plain C types only: pointers + sizes, no Go or torch types.  All byte strings
 * are big-endian as in JWK / Go's big.Int.Bytes(), except the Ed25519 public key
 * (32 raw bytes, RFC 8032 encoding).
 */
#ifndef CAPJWT_JG_H
#define CAPJWT_JG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* JWS algorithms -- jwt/algs.go:12-21 */
enum jg_alg {
  JG_ALG_NONE = 0, /* anything not in jwt/algs.go:24-35 (HS256, none, ...) -> reject */
  JG_RS256 = 1, JG_RS384 = 2, JG_RS512 = 3,
  JG_PS256 = 4, JG_PS384 = 5, JG_PS512 = 6,
  JG_ES256 = 7, JG_ES384 = 8, JG_ES512 = 9,
  JG_EDDSA = 10
};

enum jg_key_kind { JG_KEY_RSA = 1, JG_KEY_EC = 2, JG_KEY_ED25519 = 3 };
enum jg_curve { JG_P256 = 1, JG_P384 = 2, JG_P521 = 3 };

/* One public key: *rsa.PublicKey | *ecdsa.PublicKey | ed25519.PublicKey. */
typedef struct jg_key {
  int32_t kind;            /* jg_key_kind */
  int32_t curve;           /* jg_curve, EC only */
  const uint8_t* n;        /* RSA modulus, big-endian (leading zeros allowed) */
  int32_t n_len;
  uint64_t e;              /* RSA public exponent as decoded (Go rejects e<2, e>2^31-1) */
  const uint8_t* x;        /* EC X / Ed25519 public key (32 bytes) */
  const uint8_t* y;        /* EC Y */
  int32_t coord_len;       /* EC coordinate length in bytes (32/48/66) */
} jg_key;

/* One verification job.  `off`/`sig_in_len` locate the JWS signing input
 * (go-jose computeAuthData: BASE64URL(protected) '.' BASE64URL(payload), or the
 * raw payload when b64=false) inside the arena; the signature is the base64url
 * string at arena[off + sig_rel_off, +sig_b64_len) with any trailing '='
 * already trimmed by the caller (go-jose base64URLDecode).
 * The verdict is the crypto outcome for (alg, key) on those bytes. */
typedef struct jg_tok {
  uint64_t off;
  uint32_t sig_in_len;
  uint32_t sig_rel_off;
  uint32_t sig_b64_len;
  uint16_t key_idx;        /* index into the last jg_keys_load table */
  uint8_t alg;             /* jg_alg */
  uint8_t flags;           /* reserved, 0 */
} jg_tok;

/* verdict_out[i] values */
enum { JG_REJECT = 0, JG_ACCEPT = 1 };

typedef struct jg_ctx jg_ctx;
typedef struct jg_batch jg_batch;

/* Create a context on the given HIP devices (NULL/0 = device 0). */
jg_ctx* jg_create(const int* devices, int ndev);
void jg_destroy(jg_ctx* ctx);

/* Replace the key table (copied; may be reloaded on JWKS refresh -- go-oidc
 * RemoteKeySet updateKeys behind jwt/keyset.go:127).  Invalid keys (off-curve
 * EC point, Ed25519 point that does not decode, even or unusable RSA modulus,
 * e out of range) load fine and verify nothing -- the same outcome Go produces
 * per token.
 *  - A key list identical to the loaded one (same bytes, same table budget)
 *    returns 0 at once: no device work, nothing drained, staged batches stay
 *    valid.
 *  - Otherwise the new table is staged beside running verifications (no
 *    drain): work submitted before the call finishes against the old table,
 *    work submitted after it returns runs against the new one.  A key that was
 *    already loaded keeps its comb table (shared by content, no copy); a new
 *    EC / Ed25519 key gets a narrow table first (P-256 W = 20: 436 MB, about
 *    0.1 s) so it verifies as soon as this returns, and its budgeted wide table
 *    is built in the background and swapped in when complete
 *    (jg_keys_wait_tables).  CAPJWT_TABLES_SYNC=1 builds full width here.
 * Returns 0, -1 on bad arguments, or -2 when the table cannot be staged (more
 * than 256 EC keys of one curve, not enough free HBM for the new tables, a
 * device allocation or kernel failure): the previous table then stays in force
 * on every device, as go-oidc keeps its cached keys when updateKeys fails. */
int jg_keys_load(jg_ctx* ctx, const jg_key* keys, int nkeys);

/* Block until the background comb-table widening of the last jg_keys_load has
 * finished (every key verifying with its budgeted table width).  Returns 0, 1
 * when some table stayed narrower because it did not fit free HBM (see
 * jg_last_error), -1 on bad arguments. */
int jg_keys_wait_tables(jg_ctx* ctx);

/* Comb width of each loaded key's table on the context's first device (0 for
 * RSA and invalid keys): widths[0..min(n, cap)).  Returns n, the key count. */
int jg_keys_table_widths(jg_ctx* ctx, int* widths, int cap);

/* Test / A-B hook: small submissions (at most 64 jobs, every job rejected or of
 * one of the one-launch classes: ECDSA on P-256 / P-384 / P-521, EdDSA, or
 * RSA-2048 with PKCS#1 v1.5 -- RS256 / RS384 / RS512) run as one launch per
 * (class, key-table width) that does the whole verification per token --
 * enable 1: on (the default), 0: off (they take the batch chain: arena DMA,
 * plan fill, prep, scalar, point, exact, scatter), -1: unchanged.  Verdicts are
 * identical either way.  Applies to later submissions.  *launches (may be
 * NULL) receives the number of such launches this context has enqueued: the
 * counter counts launches, one per (class, width) group of a submission, not
 * tokens.  Returns 0 or -1. */
int jg_debug_small_path(jg_ctx* ctx, int enable, uint64_t* launches);

/* Test hook: the n-th device allocation of later key loads (counting from 1)
 * fails as if hipMalloc ran out of memory; 0 disables.  Returns 0 or -1. */
int jg_debug_fail_alloc(jg_ctx* ctx, int n);

/* Test hook of the degraded path (SURVEY §5 failure row): the n-th later
 * jg_submit / jg_verify_batch of this context (counting from 1) fails as a
 * device fault would -- its jg_wait returns -2 -- and the context is then
 * unusable, as after a sticky HIP error: every later submission returns -2
 * until the context is destroyed and recreated (the host layer's Engine does
 * that, re-staging its key list).  0 disables.  Returns 0 or -1. */
int jg_debug_fail_verify(jg_ctx* ctx, int n);

/* Test hook: the background upgrader widens at most n more comb tables of
 * this context (-1 = no limit, the default; CAPJWT_DEBUG_MAX_UPGRADES sets
 * the initial value), so a class can be held at mixed widths; raising it
 * resumes widening.  Returns 0 or -1. */
int jg_debug_max_upgrades(jg_ctx* ctx, int n);

/* Debug check of the key-memory lifetime rule (process-wide; also
 * CAPJWT_CHECK_LIFETIME=1): every stream that launches against a key
 * generation records an event, and releasing the generation queries them --
 * one still pending is a violation (logged to stderr).  enable: 1 on, 0 off,
 * -1 unchanged; *violations / *checked (either may be NULL) receive the
 * counts so far.  Returns 0. */
int jg_debug_lifetime_check(int enable, uint64_t* violations, uint64_t* checked);

/* Test hook: a 64-bit digest of key `key`'s current comb table on the first
 * device (0 when it has none) -- tables built at different times or on
 * different paths must agree.  Returns 0, -1 or -2. */
int jg_debug_table_digest(jg_ctx* ctx, int key, uint64_t* digest);

/* Test hook: read raw comb-table entries back from the first device.  key >= 0
 * selects that key's current table; a negative key one of the fixed-base
 * tables every token of a curve reads: JG_TABLE_P256_G, JG_TABLE_P384_G,
 * JG_TABLE_P521_G (the curve generators) or JG_TABLE_ED25519_B (the Ed25519
 * base point), which exist once a key of the curve has been loaded.  A table
 * of comb width W holds nwin windows of NE = 2^(W-1) entries; entry
 * e = w * NE + (d - 1) is d * 2^(W w) * P (P: the key's point, the generator,
 * or for an Ed25519 key -A), `stride_words` 32-bit words each:
 *   P-256          x then y, 8 little-endian 32-bit words each, canonical
 *                  Montgomery form with R = 2^280 (stride 16);
 *   P-384, P-521   x then y, L = 15 / 20 limbs of 28 bits each, canonical
 *                  Montgomery form with R = 2^(28 L) (stride 32 / 40);
 *   Ed25519        y + x, y - x, 2 d x y: three canonical values of 10
 *                  radix-2^25.5 limbs each (stride 32).
 * Words of the stride past these are padding.  The call copies n_entries
 * entries from first_entry on into out (out_words: its capacity in words) and
 * stores the table's class (the kernel class: 4 P-256, 5 P-384, 6 P-521, 7
 * Ed25519), comb width, window count and stride through the last four
 * pointers (each may be NULL; written whenever the table exists, also when
 * the range is refused).  Returns 0; -1 with jg_last_error set and nothing
 * copied for a key out of range or without a table (RSA, invalid), a
 * fixed-base table not built yet, a range past nwin * NE, or out_words too
 * small; -2 on an infrastructure error. */
#define JG_TABLE_P256_G (-1)
#define JG_TABLE_P384_G (-2)
#define JG_TABLE_P521_G (-3)
#define JG_TABLE_ED25519_B (-4)
int jg_debug_table_read(jg_ctx* ctx, int key, uint64_t first_entry, uint32_t n_entries, uint32_t* out,
                        size_t out_words, int* cls, int* width, int* nwin, int* stride_words);

/* Test hook: the number of key comb tables this context has built so far, on
 * every device (key loads and background width upgrades; a table reused from
 * the per-device cache -- same key content and width -- is not a build).
 * Returns 0 or -1. */
int jg_debug_tables_built(jg_ctx* ctx, uint64_t* built);

/* Verify ntok jobs, blocking (= jg_submit + jg_wait).  Host buffers; copied to
 * the device(s) in chunks whose H2D copies overlap the kernels of the previous
 * chunk (direct DMA when `arena` is pinned -- jg_host_alloc -- else through
 * pinned staging).  A batch whose jobs span two or more kernel classes (e.g.
 * RSA and ECDSA keys) and whose arena (16-byte aligned) lies in one
 * jg_host_alloc block is not DMAed: it runs as one class-major plan, each
 * class's token bytes gathered from the pinned arena over PCIe by a kernel,
 * costliest class first, while earlier classes compute -- when zero-copy
 * plans are on (jg_set_zero_copy; off by default, CAPJWT_ZC=1).  Returns 0 on success, -1 on bad arguments (a key_idx
 * outside the loaded table, a signing-input or signature span past
 * arena_len), -2 on an infrastructure error (see jg_last_error); per-token
 * outcomes are only in verdict_out[i] (JG_ACCEPT / JG_REJECT).  ntok == 0
 * returns 0 without touching the buffers.
 * Replaces the per-token loops of jwt/keyset.go:162-167 (staticKeySet) and
 * jwt/keyset.go:127 (go-oidc remoteKeySet) for a whole batch. */
int jg_verify_batch(jg_ctx* ctx, const uint8_t* arena, size_t arena_len,
                    const jg_tok* toks, size_t ntok, uint8_t* verdict_out);

/* Asynchronous form: jg_submit checks its arguments, queues the jobs on the
 * context's devices and returns at once with a ticket (-1 on bad arguments, -2
 * on an infrastructure error); arena, toks and verdict_out must stay valid and
 * unmodified until jg_wait(ticket) returns.  Consecutive submissions pipeline
 * back to back on each device.  The jobs themselves are validated by the
 * device workers chunk by chunk, in the same pass that plans each chunk, so a
 * bad job (a key_idx outside the table, a span past arena_len) is reported by
 * jg_wait: it returns -1 and verdict_out is then only partly written (chunks
 * before the bad one are verified; the rest are not).  jg_wait blocks until
 * the batch is complete, frees the ticket and returns 0, -1 or -2.  A batch
 * runs entirely against the key table current at submit time, even when a
 * jg_keys_load replaces it while the batch is queued. */
typedef struct jg_ticket jg_ticket;
int jg_submit(jg_ctx* ctx, const uint8_t* arena, size_t arena_len, const jg_tok* toks, size_t ntok,
              uint8_t* verdict_out, jg_ticket** ticket);
int jg_wait(jg_ctx* ctx, jg_ticket* ticket);

/* Jobs per pipeline chunk of jg_submit / jg_verify_batch (default 65536, or
 * CAPJWT_CHUNK; >= 64).  Applies to later submissions.  Returns 0 or -1. */
int jg_set_chunk(jg_ctx* ctx, size_t jobs);

/* Class-major zero-copy plans of jg_verify_batch / jg_submit (see above): on
 * (enable != 0) or off (the default unless CAPJWT_ZC=1), and the jobs per plan
 * (max_jobs >= 64; 0 keeps the current value; default 2M or CAPJWT_ZC_MAX) --
 * a longer submission runs as equal plans of at most that many jobs.  Applies
 * to later submissions.  Returns 0 or -1. */
int jg_set_zero_copy(jg_ctx* ctx, int enable, size_t max_jobs);

/* HBM (bytes per device, one total over all curves) the context may spend on
 * the comb tables of its EC and Ed25519 keys (default 32 GiB, or
 * CAPJWT_TABLE_BUDGET_GB).  The next jg_keys_load first gives every key its
 * curve's narrowest table (always allowed: P-256 W = 20, 436 MB; P-384 16,
 * 105 MB; P-521 16, 173 MB; Ed25519 16, 67 MB), then widens P-256, P-384,
 * Ed25519 and P-521 in that order, each curve to the widest width whose tables
 * for all of its keys still fit what is left: P-256 W = 26 (21.5 GB per key,
 * 20 point additions per token), 24 (5.9 GB, 21) or 22 (1.6 GB); P-384 W = 24
 * (18.3 GB), 20 (1.34 GB) or 18 (369 MB); Ed25519 24 (11.8 GB), 22 (3.2 GB),
 * 20 (872 MB) or 18 (252 MB); P-521 20 (2.26 GB) or 18 (629 MB: 30 windows)
 * -- HBM traded for fewer additions, as the shared generator tables do.  At
 * the default 32 GiB a lone P-256 key gets W = 26, 2-5 keys 24, 6-21 keys 22;
 * bench.py key_widths mirrors the rule (tests/test_bench_contract.py).
 * New tables are also sized against free HBM: a load narrows them rather than
 * fail.  Besides the budget, each device holds the generator / base-point
 * tables (about 54 GB with all four curves) for the life of the process
 * (CAPJWT_RELEASE_GTABLES=1 frees them with the last context).  Returns 0 or -1. */
int jg_set_table_budget(jg_ctx* ctx, uint64_t bytes);

const char* jg_last_error(jg_ctx* ctx);

/* Pinned host memory for arenas / job arrays (hipHostMalloc).  The block
 * carries 256 readable bytes past `bytes`, so kernels may read an arena in it
 * in place (jg_verify_batch's zero-copy plans). */
void* jg_host_alloc(size_t bytes);
void jg_host_free(void* p);

/* ---- device-resident batches (throughput measurement, pipelining) ----
 * jg_batch_stage copies a batch to the device of `device_slot` and precomputes
 * its dispatch plan (bucketing by algorithm family and key); jg_batch_run runs
 * the verify kernels on the resident inputs (no H2D) and, if verdict_out is
 * non-NULL, copies verdicts back.  jg_batch_run is asynchronous when
 * verdict_out is NULL; jg_batch_sync waits.  Consecutively staged batches of a
 * device alternate between two compute lanes on different hardware queues:
 * runs of one batch are in order, runs of two batches enqueued back to back
 * overlap on the device. */
int jg_batch_stage(jg_ctx* ctx, int device_slot, const uint8_t* arena, size_t arena_len,
                   const jg_tok* toks, size_t ntok, jg_batch** out);
int jg_batch_run(jg_ctx* ctx, jg_batch* b, uint8_t* verdict_out);
/* Enqueue one run (kernels + verdict copy into verdict_out, which must be
 * pinned -- jg_host_alloc -- and stay valid until jg_batch_sync) and return
 * without waiting: consecutive runs stream back to back on the device. */
int jg_batch_enqueue(jg_ctx* ctx, jg_batch* b, uint8_t* verdict_out);
int jg_batch_sync(jg_ctx* ctx, jg_batch* b);
void jg_batch_free(jg_ctx* ctx, jg_batch* b);

/* Per-kernel device time (ms) of the last jg_batch_run, measured with HIP
 * events on the batch's stream.  names/ms arrays of length cap; returns count. */
int jg_batch_kernel_times(jg_batch* b, const char** names, float* ms, int cap);

/* Diagnostics of the last run of a resident batch: counts[c] = tokens of kernel
 * class c (0 reject, 1-3 RSA-2K/3K/4K, 4-6 P-256/384/521, 7 Ed25519) whose
 * ECDSA comb sum hit an exceptional case of the group law and were recomputed
 * by the complete-formula path.  Returns the number of classes (8) or <0. */
int jg_batch_exceptions(jg_batch* b, uint32_t* counts, int cap);

/* ---- batched SHA-2 of byte strings ----
 * The hash of cap's OIDC hash-claim checks: oidc/id_token.go:121-135
 * (verifyHashClaim, behind IDToken.VerifyAccessToken :59 and
 * VerifyAuthorizationCode :83) hashes the access token / authorization code
 * with SHA-256, SHA-384 or SHA-512 by the id_token's alg.  Job i hashes
 * arena[off, off + len) with `fam`; digest_out receives njobs x 64 bytes, the
 * digest (32 / 48 / 64 bytes) left-aligned and zero-filled.  Blocking; runs on
 * the context's first device.  Returns 0, or <0 on bad arguments (a span past
 * arena_len, unknown fam) or an infrastructure error. */
enum jg_hash_fam { JG_SHA256 = 1, JG_SHA384 = 2, JG_SHA512 = 3 };
typedef struct jg_hjob {
  uint64_t off;
  uint32_t len;
  uint8_t fam;             /* jg_hash_fam */
  uint8_t pad_[3];
} jg_hjob;
int jg_hash_batch(jg_ctx* ctx, const uint8_t* arena, size_t arena_len,
                  const jg_hjob* jobs, size_t njobs, uint8_t* digest_out);

/* ---- batched scan of the registered claims ----
 * The claim checks of cap's Validator.Validate after the signature and the alg
 * header (jwt/jwt.go:103-201: iss / sub / jti / aud and the nbf / exp / iat
 * window), decided on the device for callers that need the verdict and not the
 * claims map.  Job i names the base64url payload segment of one token: the
 * bytes between its two dots, unpadded, at arena[off, off + len); flags is
 * reserved, 0.  `expect` is one resolved jwt.Expected for the whole call:
 *  - strs: issuer, subject, id and the audiences back to back (lengths in
 *    iss_len, sub_len, jti_len, aud_len[0..naud)); an empty string is "not
 *    expected"; at most JG_MAX_AUD audiences and JG_EXPECT_MAX_BYTES in all;
 *  - now as unix (seconds, nanoseconds in [0, 1e9));
 *  - skew_ns: the clock-skew leeway after Go's defaulting (negative -> 0,
 *    0 -> one minute);
 *  - exp_leeway_s / nbf_leeway_s: the leeways that default a missing exp / nbf,
 *    in whole seconds, after defaulting (negative -> 0, 0 -> 150 s) and
 *    Go's int64(float64) conversion.
 * code_out[i] receives a jg_claim_code: the first failing check in Validate's
 * order (no-time, iss, sub, jti, aud, nbf, exp, iat), JG_CL_OK, or JG_CL_HOST.
 * The scan is conservative: any code other than JG_CL_HOST is exactly what the
 * host's claim checks return for that payload; JG_CL_HOST means the device
 * does not decide and the caller must (a payload that is not canonical
 * base64url of one well-formed JSON object, an escape or a control byte in a
 * string, a registered claim named twice or of an unexpected type, a date that
 * is not a plain integer of at most 15 digits, ... -- DESIGN.md lists the
 * rules).
 * Blocking; runs on the context's first device on a stream of its own, so it
 * may be called while a jg_submit of another thread is in flight and does not
 * queue behind it; concurrent scans of one context run one after the other.
 * Device buffers are kept between calls.  Returns 0; -1 on bad arguments (a
 * span past arena_len, nonzero flags, more than JG_MAX_AUD audiences, expected
 * strings over JG_EXPECT_MAX_BYTES, now_nsec out of range); -2 on an
 * infrastructure error and in a context a device failure has made unusable.
 * njobs == 0 returns 0 without touching the buffers. */
#define JG_MAX_AUD 16
#define JG_EXPECT_MAX_BYTES 4096
enum jg_claim_code {
  JG_CL_OK = 0,      /* every check passed */
  JG_CL_NO_TIME = 1, /* "no issued at (iat), not before (nbf), or expiration time (exp) claims in token" */
  JG_CL_ISS = 2,     /* "invalid issuer (iss) claim" */
  JG_CL_SUB = 3,     /* "invalid subject (sub) claim" */
  JG_CL_JTI = 4,     /* "invalid ID (jti) claim" */
  JG_CL_AUD = 5,     /* "invalid audience (aud) claim: audience claim does not match any expected audience" */
  JG_CL_NBF = 6,     /* "invalid not before (nbf) claim: token not yet valid" */
  JG_CL_EXP = 7,     /* "invalid expiration time (exp) claim: token is expired" */
  JG_CL_IAT = 8,     /* "invalid issued at (iat) claim: token issued in the future" */
  JG_CL_HOST = 9     /* the device does not decide; the host must */
};
typedef struct jg_cjob {
  uint64_t off;
  uint32_t len;
  uint32_t flags;          /* reserved, 0 */
} jg_cjob;
typedef struct jg_expect {
  const uint8_t* strs;
  uint32_t iss_len, sub_len, jti_len;
  uint32_t naud;
  uint32_t aud_len[JG_MAX_AUD];
  int64_t now_sec;
  uint32_t now_nsec;
  uint32_t pad_;
  int64_t skew_ns;
  int64_t exp_leeway_s, nbf_leeway_s;
} jg_expect;
int jg_claims_scan(jg_ctx* ctx, const uint8_t* arena, size_t arena_len,
                   const jg_cjob* jobs, size_t njobs, const jg_expect* expect, uint8_t* code_out);

/* ---- the scan that also returns the registered claims ----
 * jg_claims_scan for callers that read the registered claims after the verdict
 * (the subject to authorise, the expiry to cache until): the same jobs, the same
 * `expect`, the same code_out[i] -- for the same input, always -- and with it
 * vals_out[i], what the scan read of jwt.Claims (jwt/jwt.go:107-116):
 *  - exp / nbf / iat: the payload's NumericDate values; 0 where the field is
 *    absent or null (bit f of `present` tells 0 from absent);
 *  - iss / sub / jti: the string's contents (between the quotes) as a byte span
 *    [off, off + len) of the DECODED payload.  The scan decides only payloads
 *    whose registered strings are ASCII without escapes, so those bytes are the
 *    Go string: decode characters [4 (off / 3), 4 ceil((off + len) / 3)) of the
 *    segment and cut the span out, no JSON parse.  "" has its bit set, len 0 and
 *    off = the position after the opening quote; null has its bit clear and
 *    off = len = 0;
 *  - aud: the value's text from its first byte (" or [) through its last
 *    (" or ]), and aud_n, the number of its string elements (1 for a string, k
 *    for an array of k, 0 for []); the elements are the quoted runs of the span;
 *  - present: bit f (1 iss, 2 sub, 3 jti, 4 aud, 5 exp, 6 nbf, 7 iat) is set
 *    when the payload names field f with a value other than null.
 * The record is filled for every code other than JG_CL_HOST, failures such as
 * JG_CL_EXP included; for JG_CL_HOST all 64 bytes are zero and the caller reads
 * the claims itself.
 * Everything else is jg_claims_scan's: blocking, on the context's first device
 * on the same stream of its own (extracts and scans of one context run one
 * after the other, neither waits for nor delays a jg_submit), device buffers
 * kept between calls, 0 / -1 / -2 as there, njobs == 0 returns 0 without
 * touching the buffers.  vals_out == NULL with njobs > 0 is -1. */
typedef struct jg_claims {
  int64_t  exp, nbf, iat;        /* the payload's values; 0 where absent or null */
  uint32_t iss_off, iss_len;     /* string contents (between the quotes), byte span in the DECODED payload */
  uint32_t sub_off, sub_len;
  uint32_t jti_off, jti_len;
  uint32_t aud_off, aud_len;     /* the aud value's text, from its first byte (" or [) through its last (" or ]) */
  uint32_t aud_n;                /* its string elements: 1 for a string, k for an array of k (0 for []) */
  uint32_t present;              /* bit f (F_ISS=1 .. F_IAT=7 of claims.hpp): the field was named with a non-null value */
} jg_claims;
int jg_claims_extract(jg_ctx* ctx, const uint8_t* arena, size_t arena_len,
                      const jg_cjob* jobs, size_t njobs, const jg_expect* expect,
                      uint8_t* code_out, jg_claims* vals_out);

/* ---- the scan that also returns claims the caller names ----
 * jg_claims_extract for callers that read a claim outside the registered seven
 * after the verdict (scope, roles, tenant, email; the nonce, azp and auth_time
 * of oidc/provider.go:445-506): the same jobs, the same `expect`, and
 * code_out[i] and vals_out[i] are jg_claims_extract's for the same input, byte
 * for byte, always -- selecting never changes a decision.  `select` names up to
 * JG_MAX_SELECT claims, back to back in `names`, and sel_out[i] describes them:
 *  - slot k is the top-level member whose key equals name k exactly, byte for
 *    byte (case-sensitive: the claims map is a Go map[string]interface{}, not
 *    the case-folding jwt.Claims struct).  A key at depth >= 2 never matches.
 *    Where a name occurs more than once, the last occurrence wins, as in Go's
 *    map decode.  The scan's rules already leave every payload whose keys could
 *    differ from their bytes to the host (no backslash anywhere, no byte >= 0x80
 *    in a top-level key), so no code depends on `select`.  A name may equal a
 *    registered one ("sub"): it is matched exactly in its slot and, unchanged
 *    and in any casing, by the registered logic;
 *  - JG_SEL_ABSENT: no such member; off = len = 0;
 *  - JG_SEL_STRING: a string whose bytes are all < 0x80; the span is the
 *    contents between the quotes, as for iss ("" has len 0 and off = the
 *    position after the opening quote);
 *  - JG_SEL_STRING_RAW: a string that holds a byte >= 0x80; the span runs from
 *    the opening quote through the closing quote, for the caller's JSON parser
 *    (Go replaces invalid UTF-8 with U+FFFD);
 *  - JG_SEL_NUMBER: the literal's text (at most 17 bytes, no exponent: the
 *    scan's rule);
 *  - JG_SEL_TRUE / FALSE / NULL: the literal's span (a member named with null
 *    is NULL, not ABSENT: the map holds the key with nil);
 *  - JG_SEL_ARRAY / OBJECT: from the opening bracket through its matching
 *    closing bracket.
 * Spans are byte spans [off, off + len) of the DECODED payload, as jg_claims'.
 * For JG_CL_HOST all 80 bytes of the record are zero, as the jg_claims record
 * is; for every other code, failure codes included, it is filled.  With
 * select->n == 0 every slot is ABSENT.
 * Everything else is jg_claims_extract's: blocking, on the context's first
 * device on the same stream of its own and under the same lock (selects,
 * extracts and scans of one context run one after the other, none waits for nor
 * delays a jg_submit), device buffers kept between calls, 0 / -1 / -2 as there,
 * njobs == 0 returns 0 without touching the buffers.  Also -1: select->n over
 * JG_MAX_SELECT; a name of length 0 or over JG_SELECT_NAME_MAX; a name byte
 * outside 0x20..0x7e or equal to " or \; two equal names; select, sel_out or
 * vals_out NULL with njobs > 0. */
#define JG_MAX_SELECT 8
#define JG_SELECT_NAME_MAX 64
typedef struct jg_select {          /* the caller's claim names, back to back in `names` */
  const uint8_t* names;
  uint32_t n;                       /* 0..JG_MAX_SELECT */
  uint32_t name_len[JG_MAX_SELECT];
} jg_select;
enum jg_sel_type { JG_SEL_ABSENT = 0, JG_SEL_STRING = 1, JG_SEL_STRING_RAW = 2, JG_SEL_NUMBER = 3,
                   JG_SEL_TRUE = 4, JG_SEL_FALSE = 5, JG_SEL_NULL = 6, JG_SEL_ARRAY = 7, JG_SEL_OBJECT = 8 };
typedef struct jg_selected {        /* 80 bytes: five 16-byte stores */
  uint32_t off[JG_MAX_SELECT];      /* byte span in the DECODED payload, as jg_claims' spans */
  uint32_t len[JG_MAX_SELECT];
  uint8_t  type[JG_MAX_SELECT];     /* jg_sel_type */
  uint8_t  pad_[8];                 /* zero */
} jg_selected;
int jg_claims_select(jg_ctx* ctx, const uint8_t* arena, size_t arena_len,
                     const jg_cjob* jobs, size_t njobs, const jg_expect* expect, const jg_select* select,
                     uint8_t* code_out, jg_claims* vals_out, jg_selected* sel_out);

/* ---- the three scans with an Expected per token ----
 * jg_claims_scan / jg_claims_extract / jg_claims_select for a batch whose tokens
 * are held to different jwt.Expected (several tenants or OIDC clients behind one
 * gateway): cap's Validate takes its Expected per call, and so does each job
 * here.  `expects` holds nexpect profiles, each a jg_expect as above, and in
 * this entry only jobs[i].flags is the index of job i's profile.  The mode
 * follows the outputs:
 *  - sel_out non-NULL: jg_claims_select (needs `select` and vals_out);
 *  - else vals_out non-NULL: jg_claims_extract;
 *  - else: jg_claims_scan.
 * For every job, code_out[i], vals_out[i] and sel_out[i] are what that entry
 * writes when it is called with expects[jobs[i].flags], byte for byte, always;
 * with nexpect == 1 the call is the old entry.  Profiles only differ in what
 * jg_expect holds: `select` is one name list for the call.
 * The profiles travel as one table of at most JG_MAX_PROFILES headers and
 * JG_PROFILE_POOL_BYTES string bytes in all (the kernel keeps it in 16 KiB of
 * LDS), uploaded whole on every call into one more kept device buffer.
 * Everything else is jg_claims_scan's: blocking, on the context's first device
 * on the same stream of its own and under the same lock, device buffers kept
 * between calls, njobs == 0 returns 0 without touching the buffers, -2 on an
 * infrastructure error and in a context a device failure has made unusable.
 * -1: nexpect 0 or over JG_MAX_PROFILES; a jobs[i].flags >= nexpect; a profile
 * jg_claims_scan refuses (more than JG_MAX_AUD audiences, strings over
 * JG_EXPECT_MAX_BYTES, now_nsec out of range); the profiles' strings over
 * JG_PROFILE_POOL_BYTES in total; a `select` jg_claims_select refuses; sel_out
 * without select or without vals_out; expects, jobs or code_out NULL with
 * njobs > 0; a span past arena_len. */
#define JG_MAX_PROFILES 64
#define JG_PROFILE_POOL_BYTES 8192
int jg_claims_each(jg_ctx* ctx, const uint8_t* arena, size_t arena_len,
                   const jg_cjob* jobs, size_t njobs,
                   const jg_expect* expects, uint32_t nexpect,
                   const jg_select* select,      /* NULL unless sel_out */
                   uint8_t* code_out, jg_claims* vals_out /* may be NULL */,
                   jg_selected* sel_out /* may be NULL */);

/* ---- the selecting scan for claims inside objects ----
 * jg_claims_each's selecting form for members that are not at the top level
 * (Keycloak's realm_access.roles, the cnf.jkt of RFC 9449, the act.sub of RFC
 * 8693): `paths` holds up to JG_MAX_PATHS paths of 1..JG_PATH_MAX_COMP
 * components each, a component being a name under jg_select's rules, and slot k
 * of sel_out[i] describes the value Go reaches in the claims map by walking
 * path k:
 *  - start at the top-level object; for each component, if the current value
 *    is not an object the slot is JG_SEL_ABSENT, else take the LAST member whose
 *    key equals the component byte for byte, or ABSENT if there is none: a
 *    repeated parent replaces the earlier one wholesale ({"a":{"b":1},"a":{}}
 *    is ABSENT for a/b), arrays are never descended, and component j only
 *    matches a key at depth j;
 *  - the value reached after the last component is described exactly as
 *    jg_claims_select describes a top-level member: the same jg_sel_type, the
 *    same spans, null is NULL.  A one-component path is jg_claims_select's slot
 *    for that name, byte for byte.
 * Paths may share a prefix, and one may be a prefix of another (a -> the
 * OBJECT's span, a/b -> its member).  Components are literal keys: no
 * separator is parsed, "a.b" is one component.
 * Selecting by path never changes a decision: code_out and vals_out are
 * jg_claims_each's for the same jobs and profiles, byte for byte, and no payload
 * is JG_CL_HOST because of `paths` (a payload with a backslash is HOST already; a
 * nested key with a byte >= 0x80 is not, and equals no component).  For
 * JG_CL_HOST all 80 bytes of sel_out[i] are zero; for every other code it is
 * filled; with paths->n == 0 every slot is ABSENT.
 * jobs[i].flags is the profile index.  Everything else is jg_claims_each's:
 * blocking, first device, the scan's stream and lock, kept buffers (one more for
 * the resolved paths, uploaded whole per call), -2 on an infrastructure error,
 * njobs == 0 returns 0.  -1: everything jg_claims_each refuses; paths->n over
 * JG_MAX_PATHS; an ncomp of 0 or over JG_PATH_MAX_COMP; a component jg_select
 * would refuse as a name; two equal paths; paths, vals_out or sel_out NULL with
 * njobs > 0. */
#define JG_MAX_PATHS 8
#define JG_PATH_MAX_COMP 4
typedef struct jg_paths {
  const uint8_t* names;                      /* components back to back, path by path */
  uint32_t n;                                /* 0..JG_MAX_PATHS */
  uint32_t ncomp[JG_MAX_PATHS];              /* 1..JG_PATH_MAX_COMP */
  uint32_t comp_len[JG_MAX_PATHS][JG_PATH_MAX_COMP];
} jg_paths;
int jg_claims_paths(jg_ctx* ctx, const uint8_t* arena, size_t arena_len,
                    const jg_cjob* jobs, size_t njobs,
                    const jg_expect* expects, uint32_t nexpect, const jg_paths* paths,
                    uint8_t* code_out, jg_claims* vals_out, jg_selected* sel_out);

/* ---- the scan that answers yes/no questions about claims ----
 * jg_claims_paths for callers that read a claim only to test it (does scope
 * hold orders:read, is admin among realm_access.roles, is azp this client, is
 * cnf.jkt there): the same jobs, profiles and `paths`, and instead of records
 * one mask per token.  `preds` holds up to JG_MAX_PRED predicates, each a path
 * (an index into `paths`; several predicates may name one path), an operator
 * and a value (the values back to back in `values`).  Bit k of match_out[i] is
 * set exactly when predicate k holds on the claims map the host builds for that
 * payload.  With v the value jg_claims_paths' walk reaches along paths[path[k]]
 * (objects only, never arrays; the last member of a key wins; a repeated parent
 * replaces the earlier one wholesale):
 *  - JG_PRED_EQUALS: v is a string whose bytes equal the value.  value_len 0
 *    is allowed and means "";
 *  - JG_PRED_HAS_WORD: v is a string and one of the pieces of
 *    strings.Split(v, " ") equals the value (only 0x20 separates; the RFC 6749
 *    scope form).  The value is 1..JG_PRED_VALUE_MAX bytes without a space;
 *  - JG_PRED_HAS_ELEMENT: v is an array and one of its direct elements is a
 *    string equal to the value (1..JG_PRED_VALUE_MAX bytes).  Other elements
 *    never match, nested arrays and objects are not searched, a string v does
 *    not match;
 *  - JG_PRED_PRESENT: the walk reaches a value; null counts.  value_len is 0.
 * Value bytes are 0x20..0x7e without " and \ (a name's bytes under jg_select's
 * rules).  A string that holds bytes >= 0x80 is compared as its raw bytes, so it
 * never equals an ASCII value, and its other words still count.  That is exact
 * against Go: the decoder replaces invalid UTF-8 with U+FFFD, which is three
 * bytes >= 0x80 -- never a space, never an ASCII byte -- and leaves every byte
 * < 0x80 where it is, so the ASCII runs of the Go string and of the raw bytes,
 * and the places where 0x20 splits them, are the same (a string with a
 * backslash is JG_CL_HOST already).
 * code_out[i] is jg_claims_each's code for the same jobs and profiles, byte for
 * byte, always: predicates never change a decision and no payload is
 * JG_CL_HOST because of them.  For JG_CL_HOST match_out[i] is 0; for every
 * other code, failure codes included, it is filled.  Bits n..31 are 0; with
 * preds->n == 0 every mask is 0.
 * jobs[i].flags is the profile index.  Everything else is jg_claims_paths':
 * blocking, first device, the scan's stream and lock, kept buffers (two more:
 * the resolved predicates, uploaded whole per call, and the masks), -2 on an
 * infrastructure error or an unusable context, njobs == 0 returns 0 without
 * touching the buffers.  -1: everything jg_claims_paths refuses; preds->n over
 * JG_MAX_PRED; a path[k] >= paths->n; an unknown op; a value_len outside the
 * op's range; a refused value byte; a space in a HAS_WORD value; two identical
 * predicates (same path, op and value); paths, preds, code_out or match_out
 * NULL with njobs > 0. */
#define JG_MAX_PRED 16
#define JG_PRED_VALUE_MAX 64
enum jg_pred_op {
  JG_PRED_EQUALS = 1, JG_PRED_HAS_WORD = 2, JG_PRED_HAS_ELEMENT = 3, JG_PRED_PRESENT = 4,
  /* jg_claims_match_args only; jg_claims_match refuses them as unknown */
  JG_PRED_EQUALS_ARG = 5, JG_PRED_NUM_GE = 6, JG_PRED_NUM_LE = 7, JG_PRED_NUM_GE_ARG = 8, JG_PRED_NUM_LE_ARG = 9
};
typedef struct jg_preds {
  const uint8_t* values;                     /* the predicates' values, back to back */
  uint32_t n;                                /* 0..JG_MAX_PRED */
  uint8_t  path[JG_MAX_PRED];                /* index into the call's jg_paths */
  uint8_t  op[JG_MAX_PRED];                  /* jg_pred_op */
  uint32_t value_len[JG_MAX_PRED];
} jg_preds;
int jg_claims_match(jg_ctx* ctx, const uint8_t* arena, size_t arena_len,
                    const jg_cjob* jobs, size_t njobs,
                    const jg_expect* expects, uint32_t nexpect, const jg_paths* paths, const jg_preds* preds,
                    uint8_t* code_out, uint32_t* match_out);

/* ---- predicates with an operand per token, and numeric tests ----
 * jg_claims_match for the checks whose other side differs from token to token
 * (the nonce of that request, oidc/provider.go:447; auth_time under that
 * request's max_age, :499-508; sub against the session's subject; cnf.jkt
 * against the thumbprint of the request's DPoP key): the same jobs, profiles,
 * paths, preds, code_out and match_out, and `args`, the operands of every job:
 * nstr string columns (job i's operand in column c is bytes[off, off + len) of
 * str[i * nstr + c]) and nnum columns of int64 (num[i * nnum + c]).  Five more
 * ops, with v the value the walk reaches as for the other four:
 *  - JG_PRED_EQUALS_ARG: v is a string whose bytes equal job i's operand in
 *    string column c.  value_len is 1 and the value byte is c (< nstr).  An
 *    operand of length 0 means "".  What JG_PRED_EQUALS says about bytes >= 0x80
 *    holds here too;
 *  - JG_PRED_NUM_GE / JG_PRED_NUM_LE: v is a JSON number f with f >= float64(B)
 *    (f <= float64(B)): what `f, ok := claims[..].(float64); ok && f >=
 *    float64(B)` gives in Go.  value_len is 8, the value B as a little-endian
 *    int64;
 *  - JG_PRED_NUM_GE_ARG / JG_PRED_NUM_LE_ARG: the same with B = num[i * nnum +
 *    c]; value_len is 1 and the value byte is c (< nnum).
 * Operand bytes follow a value's rules (0x20..0x7e without " and \), at most
 * JG_PRED_VALUE_MAX each; every operand of every job is checked before the
 * launch.
 * The device decides a numeric predicate only on a literal of the date form
 * -?(0|[1-9][0-9]{0,14}) (-0 counts as 0), where the integer compare is the
 * float64 compare for every int64 B.  Whenever the full path of a numeric
 * predicate reaches a number of any other accepted form (a fraction, 16 or 17
 * digits) -- also in a member that a later duplicate key replaces -- the token is
 * JG_CL_HOST, mask 0.  That is the one exception to "predicates never change a
 * code", and only a list with a numeric op can cause it; for every other token
 * code_out[i] is jg_claims_each's, byte for byte.  A string, array, literal or
 * object under a numeric predicate is bit 0, not HOST.
 * With no op >= 5 in the list the outputs are jg_claims_match's, byte for byte.
 * Everything else is jg_claims_match's (three more kept buffers: the operand
 * bytes, the span table and the numbers, uploaded per call: 8 bytes plus the
 * operand per token and string column, 8 bytes per token and number column).
 * -1: everything jg_claims_match refuses (its unknown ops are here those outside
 * 1..9); nstr or nnum over JG_MAX_ARGS; a column index past its count; a
 * value_len that is not the op's; two predicates with the same path, op and
 * column (or bound); args NULL, or bytes / str / num NULL where bytes_len / nstr
 * / nnum is not 0, with njobs > 0; and, naming the job: an operand byte a value
 * may not hold, a len over JG_PRED_VALUE_MAX, a span past bytes_len. */
#define JG_MAX_ARGS 4
typedef struct jg_sarg { uint32_t off, len; } jg_sarg;   /* bytes[off, off+len), len 0..JG_PRED_VALUE_MAX */
typedef struct jg_args {
  const uint8_t* bytes; size_t bytes_len;    /* the string operands */
  const jg_sarg* str;                        /* njobs x nstr, job-major */
  const int64_t* num;                        /* njobs x nnum, job-major */
  uint32_t nstr, nnum;                       /* 0..JG_MAX_ARGS each */
} jg_args;
int jg_claims_match_args(jg_ctx* ctx, const uint8_t* arena, size_t arena_len,
                         const jg_cjob* jobs, size_t njobs,
                         const jg_expect* expects, uint32_t nexpect, const jg_paths* paths, const jg_preds* preds,
                         const jg_args* args, uint8_t* code_out, uint32_t* match_out);

/* ---- predicates on a hash claim: at_hash, c_hash ----
 * jg_claims_match_args for the one per-request check of an OIDC callback whose
 * other side is not a value the caller holds but the hash of one
 * (oidc/id_token.go:59-145, IDToken.VerifyAccessToken / VerifyAuthorizationCode
 * -> verifyHashClaim): the claim must be a string equal to
 * base64.RawURLEncoding(SHA-2(access token)[:size/2]).  The same jobs,
 * profiles, paths, preds, args, code_out and match_out, and `hargs`: nhash hash
 * columns, job i's source in column h being bytes[off, off + len) of
 * src[i * nhash + h], hashed with `fam` (SHA-256 / 384 / 512, the family of the
 * id_token's alg; 0 = this job has no value, as under EdDSA).  A kernel of its
 * own (kernels/hash_operand.hip) hashes every source, encodes the left half of
 * the digest -- 22, 32 or 43 characters -- and writes it as that job's operand in
 * string column nstr + h of the operands jg_claims_match_args' kernel reads, on
 * the scan's stream in front of the scan: no digest comes back to the host.  Two
 * more ops, with v the value the walk reaches as for the other nine:
 *  - JG_PRED_EQUALS_HASH: v is a string whose bytes equal that encoding for job
 *    i's source in hash column h.  value_len is 1 and the value byte is h
 *    (< nhash).  Never set for a job whose fam is 0.  What JG_PRED_EQUALS_ARG
 *    says about bytes >= 0x80 and about a key named twice holds here too;
 *  - JG_PRED_IS_STRING: the walk reaches a string; "" counts, null, numbers,
 *    literals, arrays and objects do not.  value_len is 0.
 * In Go's terms (verified, err) of VerifyAccessToken is (IS_STRING &
 * EQUALS_HASH, err != nil exactly when IS_STRING holds, EQUALS_HASH does not and
 * the alg is not EdDSA).
 * Neither op changes a code and no payload is JG_CL_HOST because of them.  With
 * no op >= 10 and nhash == 0 the outputs are jg_claims_match_args', byte for
 * byte.  Source bytes are any bytes, at most JG_HASH_SRC_MAX per source; a
 * longer value is the host's to hash.
 * Everything else is jg_claims_match_args' (two more kept buffers: the source
 * bytes and the source table; the operand bytes and the span table are sized
 * for nstr + nhash columns, 44 bytes and a span per job and hash column).
 * -1: everything jg_claims_match_args refuses (its unknown ops are here those
 * outside 1..11; args may be NULL: no plain columns); nhash over
 * JG_MAX_HASH_ARGS; args->nstr + nhash over JG_MAX_ARGS; a hash column index
 * that is not below nhash; two EQUALS_HASH of one path and column; two
 * IS_STRING of one path; bytes NULL with bytes_len > 0 or src NULL with nhash >
 * 0; bytes_len of 2^32 or more; and, naming the job: a len over
 * JG_HASH_SRC_MAX, a span past bytes_len, a fam outside 0..3.  hargs may be
 * NULL: nhash 0. */
#define JG_MAX_HASH_ARGS 2
#define JG_HASH_SRC_MAX 8192
enum { JG_PRED_EQUALS_HASH = 10, JG_PRED_IS_STRING = 11 };   /* jg_claims_match_hash only */
typedef struct jg_hsrc { uint32_t off, len; uint8_t fam; uint8_t pad_[3]; } jg_hsrc;  /* fam: jg_hash_fam, or 0 = no value */
typedef struct jg_hargs {
  const uint8_t* bytes; size_t bytes_len;    /* the values to hash: any bytes */
  const jg_hsrc* src;                        /* njobs x nhash, job-major */
  uint32_t nhash, pad_;                      /* 0..JG_MAX_HASH_ARGS */
} jg_hargs;
int jg_claims_match_hash(jg_ctx* ctx, const uint8_t* arena, size_t arena_len,
                         const jg_cjob* jobs, size_t njobs,
                         const jg_expect* expects, uint32_t nexpect, const jg_paths* paths, const jg_preds* preds,
                         const jg_args* args /* may be NULL: no plain columns */,
                         const jg_hargs* hargs /* may be NULL: nhash 0 */,
                         uint8_t* code_out, uint32_t* match_out);

/* Resident sets and set-membership predicates: "is this claim one of many?" -- a
 * jti on a deny-list of revoked ids, an iss / azp / tid among the tenants a
 * gateway serves -- answered in the scan's own pass, against a hash table that
 * stays on the device between calls.
 *
 * jg_set_load builds the set `id` (0..JG_MAX_LOADED_SETS - 1) of the context from
 * n members, member k being bytes[off, off + len) of members[k], and uploads it.
 * A member is 0..JG_SET_MEMBER_MAX bytes, each in 0x20..0x7e and neither a quote
 * nor a backslash (a predicate value's rule); "" is a legal member, a repeated
 * member is folded into its first occurrence, an empty set is legal and matches
 * nothing; at most 2^24 distinct members and a pool under 2^32 bytes.  The table
 * is built on the host, deterministically from the members in their order and
 * `seed` (kernels/claim_set_build.hpp set_build), and uploaded on a stream of its own
 * to the context's FIRST device -- where every claims scan runs; nothing is
 * placed on the others.  The set is published whole: a scan captures the sets it
 * names when it starts, so a load never waits for a scan and never changes one
 * in flight, and a replaced set's memory is released when the last scan that
 * captured it has ended.  Loading an id in use replaces it.  Any failure leaves
 * the set that id named before in force: -1 (a refused member, named in
 * jg_last_error; more than 2^24 distinct members, or lengths and bytes that come
 * to 2^32 bytes of pool or more; id out of range; a needed pointer NULL), -2 (an allocation
 * failure -- jg_debug_fail_alloc reaches these allocations too -- or a HIP error).
 * jg_set_free drops the id (-1: out of range or not loaded); jg_set_info reports
 * a loaded set (-1 likewise): `generation` counts the context's successful loads
 * and is different for every one of them.  With CAPJWT_LOAD_TRACE=1 a load
 * prints its host build and its upload time on stderr, as jg_keys_load does. */
#define JG_MAX_SETS 4            /* sets one scan call may name */
#define JG_MAX_LOADED_SETS 16    /* ids 0..15 per context */
#define JG_SET_MEMBER_MAX 255
typedef struct jg_setinfo {
  uint32_t n, nslots, maxprobe, seed;        /* distinct members, table slots, longest probe run, the seed */
                                             /* nslots: a power of two >= 2n; the smallest after a load, not always after jg_set_add */
  uint64_t pool_bytes, generation;
} jg_setinfo;
int jg_set_load(jg_ctx* ctx, uint32_t id, const uint8_t* bytes, size_t bytes_len,
                const jg_sarg* members, size_t n, uint32_t seed);
int jg_set_free(jg_ctx* ctx, uint32_t id);
int jg_set_info(jg_ctx* ctx, uint32_t id, jg_setinfo* out);
/* jg_set_add adds n members to the loaded set `id` on the device (DESIGN.md
 * 10.10): a deny-list grows by a few ids without the host rebuilding and
 * uploading it whole.  Members are given and checked as jg_set_load's; one that
 * is refused is named in jg_last_error and nothing is added.  The call is
 * copy-on-write, so all that holds of a load holds of it: it builds a new table
 * and a new pool on the set stream of the first device -- the old table copied
 * device to device, or rehashed by a kernel into the smallest power of two of at
 * least 2 * (members before + n) slots when 2 * (members before + n) exceeds
 * the old slot count; the old pool copied and the new entries uploaded behind
 * it; the new entries placed by a kernel -- and publishes the result whole after
 * the stream has drained, under the old seed and a new generation.  A scan in
 * flight keeps the set it captured, an add never waits for a scan, and the old
 * memory is released when its last holder has ended.  *added (may be NULL) is
 * the number of members that were not in the set; a member already resident, or
 * given twice, takes no slot, but its entry stays behind in the pool unused:
 * pool_bytes grows by every entry handed in, and jg_set_load of the members
 * compacts it.  After adds the slot count is a power of two of at least 2 * n
 * and no longer necessarily the smallest; where among its probe run a member
 * lies depends on the order in which the device's lanes arrived, so the table is
 * not a function of the members alone (lookups do not depend on it).
 * n == 0 returns 0 and publishes nothing: the generation is unchanged.  -1: id
 * out of range or not loaded, a needed pointer NULL, a refused member, members
 * before + n over 2^24, or a pool of 2^32 bytes or more.  -2: an allocation
 * failure (jg_debug_fail_alloc reaches both allocations), a HIP error, or an
 * insertion that found no slot.  Every failure leaves the id naming what it
 * named, with the same generation.  CAPJWT_LOAD_TRACE=1 prints an add's phases
 * as a load's. */
int jg_set_add(jg_ctx* ctx, uint32_t id, const uint8_t* bytes, size_t bytes_len,
               const jg_sarg* members, size_t n, uint32_t* added /* may be NULL */);
/* Testing aid: the table (nslots pairs hash, ref) and the pool (pool_bytes / 4
 * dwords) of a loaded set, copied back from the device as they lie there, for a
 * byte-for-byte compare with the host build.  -1: not loaded, an output NULL or
 * a cap (in dwords pairs / dwords) below the set's size; -2: a HIP error. */
int jg_debug_set_read(jg_ctx* ctx, uint32_t id, uint32_t* slots_out, size_t cap_slots, uint32_t* pool_out, size_t cap_pool);

/* jg_claims_match_hash with two more ops, on sets loaded with jg_set_load; with
 * v the value the walk reaches as for the other eleven:
 *  - JG_PRED_IN_SET: v is a string whose bytes equal a member of set
 *    sets->id[value byte];
 *  - JG_PRED_ELEMENT_IN_SET: v is an array and one of its direct elements is a
 *    string equal to a member of that set.  Other elements never match, nested
 *    containers are not searched, and a string v does not match (HAS_ELEMENT's
 *    rules).
 * For both value_len is 1 and the value byte is an index below sets->nsets.  A
 * string with a byte >= 0x80 is compared raw and so equals no member; one with
 * an escape is JG_CL_HOST already.  A key named twice: the last member wins, as
 * for every op.  Neither op changes a code and no payload is JG_CL_HOST because
 * of them; the mask is 0 for HOST and bits n..31 are 0.  With no op >= 12 the
 * outputs are jg_claims_match_hash's, byte for byte (and the kernel is the one
 * that entry launches).  The scan hashes the string as it goes by and, at its
 * closing quote, looks the hash up in the set's table; a slot whose hash and
 * length agree is confirmed byte for byte against the payload, read again.
 * -1: everything jg_claims_match_hash refuses (its unknown ops are here those
 * outside 1..13); nsets over JG_MAX_SETS; an id of JG_MAX_LOADED_SETS or more,
 * or not loaded; a set index that is not one byte below nsets; two predicates
 * of the same path, op and set.  sets may be NULL: nsets 0. */
enum { JG_PRED_IN_SET = 12, JG_PRED_ELEMENT_IN_SET = 13 };   /* jg_claims_match_set only */
typedef struct jg_setargs { uint32_t nsets; uint32_t id[JG_MAX_SETS]; } jg_setargs;
int jg_claims_match_set(jg_ctx* ctx, const uint8_t* arena, size_t arena_len,
                        const jg_cjob* jobs, size_t njobs,
                        const jg_expect* expects, uint32_t nexpect, const jg_paths* paths, const jg_preds* preds,
                        const jg_args* args /* may be NULL: no plain columns */,
                        const jg_hargs* hargs /* may be NULL: nhash 0 */,
                        const jg_setargs* sets /* may be NULL: nsets 0 */,
                        uint8_t* code_out, uint32_t* match_out);

/* Library build information (gfx target, version). */
const char* jg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CAPJWT_JG_H */
