// set_add_stub.cpp -- tests/host_match_set/match_set_stub.cpp (a stand-in for
// libcapjwt.so's C ABI with resident sets and their scan on the CPU) plus
// jg_set_add: the CPU build of the insertion and rehash steps of
// kernels/claim_set_insert.hpp (tests/host_unit/claim_set_add_cpu.hpp), published
// copy-on-write as the runtime does, with a switch that fails it; and a switch
// that loses the context: the next scan drops every resident set and fails as a
// device fault does, so the host layer recovers.  For ClaimSet::Add without a GPU
// (set_add.cpp, tests/test_host_set_add.py).
//
// -DNO_SET_ADD leaves jg_set_add out, as an older library would.
#define jg_claims_match_set stub_claims_match_set_inner
#include "../host_match_set/match_set_stub.cpp"
#undef jg_claims_match_set

#include "../host_unit/claim_set_add_cpu.hpp"

extern "C" {
int set_add_stub_calls = 0;                   // successful jg_set_add calls so far
int set_add_stub_given = 0;                   // members handed to them
int set_add_stub_fail = 0;                    // != 0: jg_set_add returns -2
int set_add_stub_lose = 0;                    // != 0: the next scan loses the context
int set_add_stub_present =
#ifdef NO_SET_ADD
    0;
#else
    1;
#endif

int jg_claims_match_set(jg_ctx* ctx, const uint8_t* arena, size_t arena_len, const jg_cjob* jobs, size_t njobs,
                        const jg_expect* expects, uint32_t nexpect, const jg_paths* paths, const jg_preds* preds,
                        const jg_args* args, const jg_hargs* hargs, const jg_setargs* sets, uint8_t* code_out,
                        uint32_t* match_out) {
  if (set_add_stub_lose) {
    set_add_stub_lose = 0;
    for (auto& s : g_sets) s.reset();
    return -2;
  }
  return stub_claims_match_set_inner(ctx, arena, arena_len, jobs, njobs, expects, nexpect, paths, preds, args, hargs, sets,
                                     code_out, match_out);
}

#ifndef NO_SET_ADD
int jg_set_add(jg_ctx*, uint32_t id, const uint8_t* bytes, size_t bytes_len, const jg_sarg* members, size_t n,
               uint32_t* added) {
  if (id >= JG_MAX_LOADED_SETS || !g_sets[id] || (n && !members)) return -1;
  if (n == 0) {
    if (added) *added = 0;
    return 0;
  }
  if (set_add_stub_fail) return -2;
  auto s = std::make_shared<StubSet>(*g_sets[id]);    // copy-on-write: a scan that holds the old one keeps it
  size_t bad = 0;
  uint32_t cnt = 0;
  const int rc = jgset::set_add_cpu(&s->built, bytes, bytes_len, members, n, &cnt, &bad);
  if (rc != 0) return rc == -2 ? -2 : -1;
  s->generation = ++g_generation;
  g_sets[id] = s;
  ++set_add_stub_calls;
  set_add_stub_given += (int)n;
  if (added) *added = cnt;
  return 0;
}
#endif
}
