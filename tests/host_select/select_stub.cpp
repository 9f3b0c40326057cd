// select_stub.cpp -- tests/host_registered/accept_stub.cpp (a stand-in for
// libcapjwt.so's C ABI whose verify accepts every job and whose claims scans run
// the CPU build of the device's decision functions) plus jg_claims_select, which
// runs the CPU build of claims_select (kernels/claims.hpp).  For the host merge
// of Validator::SelectBatch without a GPU (select.cpp, tests/test_host_select.py).
//
// -DNO_SELECT leaves jg_claims_select out, as an older verifier library would.
#include "../host_registered/accept_stub.cpp"

#ifndef NO_SELECT
extern "C" int jg_claims_select(jg_ctx*, const uint8_t* arena, size_t, const jg_cjob* jobs, size_t njobs,
                                const jg_expect* expect, const jg_select* select, uint8_t* code_out,
                                jg_claims* vals_out, jg_selected* sel_out) {
  auto E = std::make_unique<jgclaims::Expect>();
  auto S = std::make_unique<jgclaims::Select>();
  if (!select || !jgclaims::resolve(*expect, E.get()) || !jgclaims::resolve_select(*select, S.get())) return -1;
  for (size_t i = 0; i < njobs; ++i) {
    ByteSrc src{arena + jobs[i].off, jobs[i].len};
    code_out[i] = jgclaims::claims_select(src, src.len, *E, *S, &vals_out[i], &sel_out[i]);
  }
  return 0;
}
#endif
