/*
 * tokgen -- synthetic signed-JWT generator for bench.py and the large-batch
 * GPU tests (input generation only; never on the measured path, never the
 * checker).  Signs with OpenSSL libcrypto, multi-threaded.
 *
 *   tokgen <ALG> <count> <threads> <out.txt> <key.pem> [key.pem ...]
 *
 * Token i uses key i % nkeys; header {"alg":ALG,"kid":"kid-KK","typ":"JWT"},
 * payload shaped like cap's testJWTClaims (jwt/keyset_test.go:666-677) with
 * jti = i (TOKGEN_PAD / TOKGEN_EXTRA / TOKGEN_OIDC add members).  One token per line.  PS* use salt length = hash length (go-jose).
 * RS*, ES* and EdDSA tokens are the same bytes on every run (ES* nonces are
 * derived, see es_sign); PS* salts are random.
 */
#include <openssl/bn.h>
#include <openssl/ecdsa.h>
#include <openssl/evp.h>
#include <openssl/hmac.h>
#include <openssl/pem.h>
#include <openssl/rsa.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const char B64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_";

static size_t b64url(const unsigned char* in, size_t n, char* out) {
  size_t o = 0, i = 0;
  for (; i + 3 <= n; i += 3) {
    unsigned v = (unsigned)in[i] << 16 | (unsigned)in[i + 1] << 8 | in[i + 2];
    out[o++] = B64[v >> 18]; out[o++] = B64[(v >> 12) & 63]; out[o++] = B64[(v >> 6) & 63]; out[o++] = B64[v & 63];
  }
  if (n - i == 1) {
    unsigned v = (unsigned)in[i] << 16;
    out[o++] = B64[v >> 18]; out[o++] = B64[(v >> 12) & 63];
  } else if (n - i == 2) {
    unsigned v = (unsigned)in[i] << 16 | (unsigned)in[i + 1] << 8;
    out[o++] = B64[v >> 18]; out[o++] = B64[(v >> 12) & 63]; out[o++] = B64[(v >> 6) & 63];
  }
  out[o] = 0;
  return o;
}

typedef struct {
  const char* alg;
  EVP_PKEY** keys;
  int nkeys;
  long lo, hi;
  char** out;
  int kid_base;           /* TOKGEN_KID_BASE: first kid number ("kid-NN") */
} job;

static const EVP_MD* alg_md(const char* alg) {
  if (!strcmp(alg, "EdDSA")) return NULL;
  const char* h = alg + 2;
  if (!strcmp(h, "256")) return EVP_sha256();
  if (!strcmp(h, "384")) return EVP_sha384();
  return EVP_sha512();
}

static int es_size(const char* alg) {
  return !strcmp(alg, "ES256") ? 32 : !strcmp(alg, "ES384") ? 48 : 66;
}

/* ES*: r || s with a nonce derived from the key, the digest and `salt`
 * (HMAC-SHA512 in counter mode, reduced mod n - 1, plus 1), so a run's tokens
 * are the same bytes every time -- two builds of the library can be compared
 * verdict for verdict on identical inputs.  TOKGEN_NONCE_SALT=text gives
 * another set of signatures over the same signing inputs.  Test input only:
 * not RFC 6979, not constant time. */
static void es_sign(EC_KEY* ec, const EVP_MD* md, const char* msg, size_t mlen, int sz, const char* salt,
                    unsigned char* raw) {
  unsigned char dg[EVP_MAX_MD_SIZE], dk[200], kb[128], mac[64], in[EVP_MAX_MD_SIZE + 1 + 64];
  const size_t sn = strnlen(salt, 64);
  unsigned dl = 0, ml = 0;
  if (EVP_Digest(msg, mlen, dg, &dl, md, NULL) != 1) { fprintf(stderr, "es digest\n"); exit(2); }
  const EC_GROUP* g = EC_KEY_get0_group(ec);
  const int dn = BN_bn2binpad(EC_KEY_get0_private_key(ec), dk, sz);
  memcpy(in, dg, dl);
  memcpy(in + dl + 1, salt, sn);
  for (int c = 0; c < 2; ++c) {
    in[dl] = (unsigned char)c;
    if (dn != sz || !HMAC(EVP_sha512(), dk, dn, in, dl + 1 + sn, mac, &ml) || ml != 64) { fprintf(stderr, "es nonce\n"); exit(2); }
    memcpy(kb + 64 * c, mac, 64);
  }
  BN_CTX* bc = BN_CTX_new();
  BIGNUM *k = BN_bin2bn(kb, sizeof kb, NULL), *n1 = BN_dup(EC_GROUP_get0_order(g)), *r = BN_new(), *kinv = BN_new();
  EC_POINT* pt = EC_POINT_new(g);
  BN_sub_word(n1, 1);
  if (!BN_mod(k, k, n1, bc) || !BN_add_word(k, 1) || EC_POINT_mul(g, pt, k, NULL, NULL, bc) != 1 ||
      EC_POINT_get_affine_coordinates(g, pt, r, NULL, bc) != 1 || !BN_mod(r, r, EC_GROUP_get0_order(g), bc) ||
      BN_is_zero(r) || !BN_mod_inverse(kinv, k, EC_GROUP_get0_order(g), bc)) { fprintf(stderr, "es point\n"); exit(2); }
  ECDSA_SIG* es = ECDSA_do_sign_ex(dg, (int)dl, kinv, r, ec);
  if (!es) { fprintf(stderr, "es sign\n"); exit(2); }
  const BIGNUM *sr, *ss;
  ECDSA_SIG_get0(es, &sr, &ss);
  BN_bn2binpad(sr, raw, sz);
  BN_bn2binpad(ss, raw + sz, sz);
  ECDSA_SIG_free(es);
  EC_POINT_free(pt);
  BN_free(k); BN_free(n1); BN_free(r); BN_free(kinv);
  BN_CTX_free(bc);
}

static void* worker(void* arg) {
  job* j = (job*)arg;
  /* TOKGEN_PAD=n: a "pad" claim of n 'x' bytes (long signing inputs) */
  const char* pe = getenv("TOKGEN_PAD");
  const size_t padn = pe ? (size_t)atol(pe) : 0;
  const char* salt = getenv("TOKGEN_NONCE_SALT");
  if (!salt) salt = "";
  /* TOKGEN_EXTRA=text: further members, written as they are in front of "sub"
   * (e.g. "roles":["admin"],"scope":"read write", -- with the trailing comma) */
  const char* extra = getenv("TOKGEN_EXTRA");
  if (!extra) extra = "";
  /* TOKGEN_OIDC=1: token i also carries "nonce":"n-<i as 20 hex digits>" (22 bytes, its own) and
   * "auth_time":1611699344 - i % 3600, in front of TOKGEN_EXTRA's members.
   * TOKGEN_OIDC=2: and "at_hash", the left half of the alg's SHA-2 of the access token "ya29.<i as 35 hex
   * digits>" (40 bytes, its own) as unpadded base64url (oidc/id_token.go verifyHashClaim); EdDSA: SHA-512 */
  const char* oe = getenv("TOKGEN_OIDC");
  const int oidc = oe ? (int)atol(oe) : 0;
  char oidcv[192] = "";
  /* TOKGEN_TENANTS=P: token i belongs to tenant i % P, with an issuer and an
   * audience of its own of the default ones' lengths ("https://t07.example/",
   * "c07.example.com"); unset or 0: the default issuer and audience */
  const char* te = getenv("TOKGEN_TENANTS");
  const long tenants = te ? atol(te) : 0;
  char iss[64] = "https://example.com/", aud[64] = "www.example.com";
  const size_t cap = 512 + sizeof oidcv + padn + strlen(extra);
  char hdr[256], hb[512], sb[1500];
  char* pay = malloc(cap);
  char* pb = malloc(2 * cap + 8);
  char* padv = malloc(padn + 1);
  memset(padv, 'x', padn);
  padv[padn] = 0;
  unsigned char sig[1024], raw[200];
  EC_KEY** ecs = calloc((size_t)j->nkeys, sizeof(EC_KEY*));     /* this thread's copies, made at first use */
  for (long i = j->lo; i < j->hi; ++i) {
    const int k = (int)(i % j->nkeys);
    if (tenants > 0) {
      snprintf(iss, sizeof iss, "https://t%02ld.example/", i % tenants);
      snprintf(aud, sizeof aud, "c%02ld.example.com", i % tenants);
    }
    snprintf(hdr, sizeof hdr, "{\"alg\":\"%s\",\"kid\":\"kid-%02d\",\"typ\":\"JWT\"}", j->alg, j->kid_base + k);
    if (oidc) snprintf(oidcv, sizeof oidcv, "\"nonce\":\"n-%020lx\",\"auth_time\":%ld,", i, 1611699344L - i % 3600);
    if (oidc == 2) {
      char at[48], ah[96];
      unsigned char dg[EVP_MAX_MD_SIZE];
      unsigned dl = 0;
      snprintf(at, sizeof at, "ya29.%035lx", i);
      const EVP_MD* hm = alg_md(j->alg);
      if (EVP_Digest(at, strlen(at), dg, &dl, hm ? hm : EVP_sha512(), NULL) != 1) { fprintf(stderr, "at_hash digest\n"); exit(2); }
      ah[b64url(dg, dl / 2, ah)] = 0;
      const size_t ol = strlen(oidcv);
      snprintf(oidcv + ol, sizeof oidcv - ol, "\"at_hash\":\"%s\",", ah);
    }
    if (padn)
      snprintf(pay, cap,
               "{\"aud\":[\"%s\"],\"exp\":1611699944,\"iat\":1611699344,"
               "\"iss\":\"%s\",\"jti\":\"%ld\",\"nbf\":1611699344,\"pad\":\"%s\","
               "%s%s\"sub\":\"alice@example.com\"}", aud, iss, i, padv, oidcv, extra);
    else
      snprintf(pay, cap,
               "{\"aud\":[\"%s\"],\"exp\":1611699944,\"iat\":1611699344,"
               "\"iss\":\"%s\",\"jti\":\"%ld\",\"nbf\":1611699344,%s%s\"sub\":\"alice@example.com\"}",
               aud, iss, i, oidcv, extra);
    size_t hl = b64url((const unsigned char*)hdr, strlen(hdr), hb);
    size_t pl = b64url((const unsigned char*)pay, strlen(pay), pb);
    char* si = malloc(hl + pl + 2);
    memcpy(si, hb, hl); si[hl] = '.'; memcpy(si + hl + 1, pb, pl); si[hl + pl + 1] = 0;
    const size_t slen_in = hl + pl + 1;
    const unsigned char* s = sig;
    size_t n;
    if (j->alg[0] == 'E' && j->alg[1] == 'S') {             /* r || s, nonce from key and digest */
      const int sz = es_size(j->alg);
      if (!ecs[k] && !(ecs[k] = EVP_PKEY_get1_EC_KEY(j->keys[k]))) { fprintf(stderr, "not an EC key\n"); exit(2); }
      es_sign(ecs[k], alg_md(j->alg), si, slen_in, sz, salt, raw);
      s = raw;
      n = 2 * (size_t)sz;
    } else {
      EVP_MD_CTX* mc = EVP_MD_CTX_new();
      EVP_PKEY_CTX* pc = NULL;
      size_t sl = sizeof sig;
      if (EVP_DigestSignInit(mc, &pc, alg_md(j->alg), NULL, j->keys[k]) != 1) { fprintf(stderr, "init\n"); exit(2); }
      if (j->alg[0] == 'P') {
        EVP_PKEY_CTX_set_rsa_padding(pc, RSA_PKCS1_PSS_PADDING);
        EVP_PKEY_CTX_set_rsa_pss_saltlen(pc, RSA_PSS_SALTLEN_DIGEST);
      }
      if (EVP_DigestSign(mc, sig, &sl, (const unsigned char*)si, slen_in) != 1) { fprintf(stderr, "sign\n"); exit(2); }
      EVP_MD_CTX_free(mc);
      n = sl;
    }
    size_t bl = b64url(s, n, sb);
    char* tok = malloc(slen_in + bl + 2);
    memcpy(tok, si, slen_in); tok[slen_in] = '.'; memcpy(tok + slen_in + 1, sb, bl + 1);
    free(si);
    j->out[i] = tok;
  }
  free(pay);
  free(pb);
  free(padv);
  for (int k = 0; k < j->nkeys; ++k) EC_KEY_free(ecs[k]);
  free(ecs);
  return NULL;
}

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: tokgen ALG count threads out.txt key.pem...\n");
    return 2;
  }
  const char* alg = argv[1];
  long count = atol(argv[2]);
  int threads = atoi(argv[3]);
  if (threads < 1) threads = 1;
  int nkeys = argc - 5;
  EVP_PKEY** keys = calloc((size_t)nkeys, sizeof(EVP_PKEY*));
  for (int i = 0; i < nkeys; ++i) {
    FILE* f = fopen(argv[5 + i], "r");
    if (!f) { perror(argv[5 + i]); return 2; }
    keys[i] = PEM_read_PrivateKey(f, NULL, NULL, NULL);
    fclose(f);
    if (!keys[i]) { fprintf(stderr, "bad key %s\n", argv[5 + i]); return 2; }
  }
  char** out = calloc((size_t)count, sizeof(char*));
  pthread_t* th = calloc((size_t)threads, sizeof(pthread_t));
  job* js = calloc((size_t)threads, sizeof(job));
  for (int t = 0; t < threads; ++t) {
    const char* kb = getenv("TOKGEN_KID_BASE");
    js[t] = (job){alg, keys, nkeys, count * t / threads, count * (t + 1) / threads, out, kb ? atoi(kb) : 0};
    pthread_create(&th[t], NULL, worker, &js[t]);
  }
  for (int t = 0; t < threads; ++t) pthread_join(th[t], NULL);
  FILE* f = fopen(argv[4], "w");
  for (long i = 0; i < count; ++i) { fputs(out[i], f); fputc('\n', f); free(out[i]); }
  fclose(f);
  return 0;
}
