// match_args_stub.cpp -- tests/host_match/match_stub.cpp (a stand-in for
// libcapjwt.so's C ABI whose verify accepts every job and whose claims scans run
// the CPU build of the device's decision functions) plus jg_claims_match_args,
// which runs the CPU build of resolve_paths, resolve_arg_preds, arg_operands_ok
// and claims_match_args (kernels/claims.hpp) and refuses what the ABI refuses.
// For the host layer of the MatchArgs entries without a GPU (match_args.cpp,
// tests/test_host_match_args.py).  It counts its calls and the jobs it scanned,
// and keeps the -1 it last returned, so the driver can see that no refused
// operand reaches the ABI.
#include "../host_match/match_stub.cpp"

extern "C" {
int match_args_stub_calls = 0;                // jg_claims_match_args calls so far
int match_args_stub_refused = 0;              // ... that returned -1
}

namespace {
struct StubArgs {
  const jg_args* a;
  size_t i;
  uint32_t nstr() const { return a->nstr; }
  uint32_t slen(uint32_t c) const { return a->str[i * a->nstr + c].len; }
  uint32_t word(uint32_t c, uint32_t p) const {
    const jg_sarg& s = a->str[i * a->nstr + c];
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4; ++k)
      if (p + k < s.len) w |= (uint32_t)a->bytes[s.off + p + k] << (8 * k);
    return w;
  }
  int64_t bound(uint32_t c) const { return a->num[i * a->nnum + c]; }
};
}  // namespace

extern "C" int jg_claims_match_args(jg_ctx*, const uint8_t* arena, size_t arena_len, const jg_cjob* jobs, size_t njobs,
                                    const jg_expect* expects, uint32_t nexpect, const jg_paths* paths,
                                    const jg_preds* preds, const jg_args* args, uint8_t* code_out, uint32_t* match_out) {
  ++match_args_stub_calls;
  const auto refuse = [] { ++match_args_stub_refused; return -1; };
  if (!expects || (njobs > 0 && (!jobs || !code_out || !paths || !preds || !match_out || !args))) return refuse();
  if (njobs == 0) return 0;
  auto T = std::make_unique<jgclaims::Profiles>();
  auto P = std::make_unique<jgclaims::Paths>();
  auto Q = std::make_unique<jgclaims::ArgPreds>();
  if (!jgclaims::resolve_profiles(expects, nexpect, T.get())) return refuse();
  if (!jgclaims::resolve_paths(*paths, P.get())) return refuse();
  if (!jgclaims::resolve_arg_preds(*preds, *P, args->nstr, args->nnum, Q.get())) return refuse();
  if ((args->bytes_len && !args->bytes) || (args->nstr && !args->str) || (args->nnum && !args->num)) return refuse();
  for (size_t i = 0; i < njobs; ++i) {
    if (jobs[i].flags >= nexpect || jobs[i].off > arena_len || jobs[i].len > arena_len - jobs[i].off) return refuse();
    if (!jgclaims::arg_operands_ok(*args, i)) return refuse();
  }
  for (size_t i = 0; i < njobs; ++i) {
    ByteSrc src{arena + jobs[i].off, jobs[i].len};
    const StubArgs A{args, i};
    code_out[i] = jgclaims::claims_match_args(src, src.len, *T, jobs[i].flags, *P, *Q, A, &match_out[i]);
  }
  return 0;
}
