// accept_stub.cpp -- a stand-in for libcapjwt.so's C ABI for the host merge of
// Validator::RegisteredBatch without a GPU (registered.cpp,
// tests/test_host_registered.py): its verify accepts every job, and its claims
// scans run the CPU build of the device's decision functions
// (kernels/claims.hpp).  Verifies nothing.
//
// -DNO_EXTRACT leaves jg_claims_extract out, as an older verifier library would.
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../cap_amd/csrc/kernels/claims.hpp"
#include "../../include/jg.h"

struct jg_ctx {
  int unused;
};

namespace {
struct ByteSrc {
  const uint8_t* p;
  uint32_t len;
  uint32_t word(uint32_t g) {
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4; ++k)
      if (4 * g + k < len) w |= (uint32_t)p[4 * g + k] << (8 * k);
    return w;
  }
};
}  // namespace

extern "C" {
jg_ctx* jg_create(const int*, int) { return new jg_ctx{0}; }
void jg_destroy(jg_ctx* c) { delete c; }
const char* jg_last_error(jg_ctx*) { return ""; }
int jg_keys_load(jg_ctx*, const jg_key*, int) { return 0; }
int jg_keys_wait_tables(jg_ctx*) { return 0; }
void* jg_host_alloc(size_t n) { return std::malloc(n ? n : 1); }
void jg_host_free(void* p) { std::free(p); }
int jg_verify_batch(jg_ctx*, const uint8_t*, size_t, const jg_tok*, size_t n, uint8_t* verdicts) {
  std::memset(verdicts, 1, n);
  return 0;
}
struct jg_ticket {
  int rc;
};
int jg_submit(jg_ctx*, const uint8_t*, size_t, const jg_tok*, size_t n, uint8_t* verdicts, jg_ticket** t) {
  std::memset(verdicts, 1, n);
  *t = new jg_ticket{0};
  return 0;
}
int jg_wait(jg_ctx*, jg_ticket* t) {
  const int rc = t->rc;
  delete t;
  return rc;
}
int jg_debug_fail_verify(jg_ctx*, int) { return 0; }
int jg_hash_batch(jg_ctx*, const uint8_t*, size_t, const jg_hjob*, size_t, uint8_t*) { return -2; }

int jg_claims_scan(jg_ctx*, const uint8_t* arena, size_t, const jg_cjob* jobs, size_t njobs, const jg_expect* expect,
                   uint8_t* code_out) {
  auto E = std::make_unique<jgclaims::Expect>();
  if (!jgclaims::resolve(*expect, E.get())) return -1;
  for (size_t i = 0; i < njobs; ++i) {
    ByteSrc src{arena + jobs[i].off, jobs[i].len};
    code_out[i] = jgclaims::claims_decide(src, src.len, *E);
  }
  return 0;
}

#ifndef NO_EXTRACT
int jg_claims_extract(jg_ctx*, const uint8_t* arena, size_t, const jg_cjob* jobs, size_t njobs,
                      const jg_expect* expect, uint8_t* code_out, jg_claims* vals_out) {
  auto E = std::make_unique<jgclaims::Expect>();
  if (!jgclaims::resolve(*expect, E.get())) return -1;
  for (size_t i = 0; i < njobs; ++i) {
    ByteSrc src{arena + jobs[i].off, jobs[i].len};
    code_out[i] = jgclaims::claims_extract(src, src.len, *E, &vals_out[i]);
  }
  return 0;
}
#endif
}
