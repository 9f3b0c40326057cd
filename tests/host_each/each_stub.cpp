// each_stub.cpp -- tests/host_select/select_stub.cpp (a stand-in for
// libcapjwt.so's C ABI whose verify accepts every job and whose claims scans run
// the CPU build of the device's decision functions) plus jg_claims_each, which
// runs the CPU build of resolve_profiles and the *_each functions
// (kernels/claims.hpp) and refuses what the ABI refuses.  For the host layer of
// the Validator::*Each entries without a GPU (each.cpp, tests/test_host_each.py).
// It counts its calls, so the driver can see one scan call per batch.
//
// -DNO_EACH leaves jg_claims_each out, as an older verifier library would.
#include "../host_select/select_stub.cpp"

extern "C" {
int each_stub_calls = 0;                      // jg_claims_each calls so far
int each_stub_profiles = 0;                   // nexpect of the last one
}

#ifndef NO_EACH
extern "C" int jg_claims_each(jg_ctx*, const uint8_t* arena, size_t arena_len, const jg_cjob* jobs, size_t njobs,
                              const jg_expect* expects, uint32_t nexpect, const jg_select* select, uint8_t* code_out,
                              jg_claims* vals_out, jg_selected* sel_out) {
  ++each_stub_calls;
  each_stub_profiles = (int)nexpect;
  if (!expects || (njobs > 0 && (!jobs || !code_out)) || (sel_out && (!select || !vals_out))) return -1;
  if (njobs == 0) return 0;
  auto T = std::make_unique<jgclaims::Profiles>();
  auto S = std::make_unique<jgclaims::Select>();
  if (!jgclaims::resolve_profiles(expects, nexpect, T.get())) return -1;
  if (sel_out && !jgclaims::resolve_select(*select, S.get())) return -1;
  for (size_t i = 0; i < njobs; ++i)
    if (jobs[i].flags >= nexpect || jobs[i].off > arena_len || jobs[i].len > arena_len - jobs[i].off) return -1;
  for (size_t i = 0; i < njobs; ++i) {
    ByteSrc src{arena + jobs[i].off, jobs[i].len};
    const uint32_t p = jobs[i].flags;
    if (sel_out) code_out[i] = jgclaims::claims_select_each(src, src.len, *T, p, *S, &vals_out[i], &sel_out[i]);
    else if (vals_out) code_out[i] = jgclaims::claims_extract_each(src, src.len, *T, p, &vals_out[i]);
    else code_out[i] = jgclaims::claims_decide_each(src, src.len, *T, p);
  }
  return 0;
}
#endif
