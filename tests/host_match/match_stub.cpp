// match_stub.cpp -- tests/host_paths/paths_stub.cpp (a stand-in for
// libcapjwt.so's C ABI whose verify accepts every job and whose claims scans run
// the CPU build of the device's decision functions) plus jg_claims_match, which
// runs the CPU build of resolve_paths, resolve_preds and claims_match_each
// (kernels/claims.hpp) and refuses what the ABI refuses.  For the host layer of
// the Match entries without a GPU (match.cpp, tests/test_host_match_batch.py).
// It counts its calls, so the driver can see which entry a call went to.
//
// -DNO_MATCH leaves jg_claims_match out, as an older verifier library would.
#include "../host_paths/paths_stub.cpp"

extern "C" {
int match_stub_calls = 0;                     // jg_claims_match calls so far
}

#ifndef NO_MATCH
extern "C" int jg_claims_match(jg_ctx*, const uint8_t* arena, size_t arena_len, const jg_cjob* jobs, size_t njobs,
                               const jg_expect* expects, uint32_t nexpect, const jg_paths* paths, const jg_preds* preds,
                               uint8_t* code_out, uint32_t* match_out) {
  ++match_stub_calls;
  if (!expects || (njobs > 0 && (!jobs || !code_out || !paths || !preds || !match_out))) return -1;
  if (njobs == 0) return 0;
  auto T = std::make_unique<jgclaims::Profiles>();
  auto P = std::make_unique<jgclaims::Paths>();
  auto Q = std::make_unique<jgclaims::Preds>();
  if (!jgclaims::resolve_profiles(expects, nexpect, T.get())) return -1;
  if (!jgclaims::resolve_paths(*paths, P.get())) return -1;
  if (!jgclaims::resolve_preds(*preds, *P, Q.get())) return -1;
  for (size_t i = 0; i < njobs; ++i)
    if (jobs[i].flags >= nexpect || jobs[i].off > arena_len || jobs[i].len > arena_len - jobs[i].off) return -1;
  for (size_t i = 0; i < njobs; ++i) {
    ByteSrc src{arena + jobs[i].off, jobs[i].len};
    code_out[i] = jgclaims::claims_match_each(src, src.len, *T, jobs[i].flags, *P, *Q, &match_out[i]);
  }
  return 0;
}
#endif
