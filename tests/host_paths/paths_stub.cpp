// paths_stub.cpp -- tests/host_each/each_stub.cpp (a stand-in for libcapjwt.so's
// C ABI whose verify accepts every job and whose claims scans run the CPU build
// of the device's decision functions) plus jg_claims_paths, which runs the CPU
// build of resolve_paths and claims_paths_each (kernels/claims.hpp) and refuses
// what the ABI refuses.  For the host layer of the Select entries by path
// without a GPU (paths.cpp, tests/test_host_paths.py).  It counts its calls, so
// the driver can see which entry a call went to.
//
// -DNO_PATHS leaves jg_claims_paths out, as an older verifier library would.
#include "../host_each/each_stub.cpp"

extern "C" {
int paths_stub_calls = 0;                     // jg_claims_paths calls so far
}

#ifndef NO_PATHS
extern "C" int jg_claims_paths(jg_ctx*, const uint8_t* arena, size_t arena_len, const jg_cjob* jobs, size_t njobs,
                               const jg_expect* expects, uint32_t nexpect, const jg_paths* paths, uint8_t* code_out,
                               jg_claims* vals_out, jg_selected* sel_out) {
  ++paths_stub_calls;
  if (!expects || (njobs > 0 && (!jobs || !code_out || !paths || !vals_out || !sel_out))) return -1;
  if (njobs == 0) return 0;
  auto T = std::make_unique<jgclaims::Profiles>();
  auto P = std::make_unique<jgclaims::Paths>();
  if (!jgclaims::resolve_profiles(expects, nexpect, T.get())) return -1;
  if (!jgclaims::resolve_paths(*paths, P.get())) return -1;
  for (size_t i = 0; i < njobs; ++i)
    if (jobs[i].flags >= nexpect || jobs[i].off > arena_len || jobs[i].len > arena_len - jobs[i].off) return -1;
  for (size_t i = 0; i < njobs; ++i) {
    ByteSrc src{arena + jobs[i].off, jobs[i].len};
    code_out[i] = jgclaims::claims_paths_each(src, src.len, *T, jobs[i].flags, *P, &vals_out[i], &sel_out[i]);
  }
  return 0;
}
#endif
