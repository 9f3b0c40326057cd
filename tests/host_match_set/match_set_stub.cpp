// match_set_stub.cpp -- tests/host_match_hash/match_hash_stub.cpp (a stand-in for
// libcapjwt.so's C ABI whose verify accepts every job and whose claims scans run
// the CPU build of the device's functions) plus the resident sets: jg_set_load /
// jg_set_free / jg_set_info keep sets built by kernels/claim_set_build.hpp
// set_build(), with a switch to make a load fail as an allocation failure does,
// and jg_claims_match_set runs the CPU build of resolve_arg_preds with the set
// ops and claims_match_set, and refuses what the ABI refuses.  For the host layer
// of the MatchArgs entries with InSet / AnyElementIn without a GPU (match_set.cpp,
// tests/test_host_match_set.py).
#include "../host_match_hash/match_hash_stub.cpp"

#include <memory>

#include "../../cap_amd/csrc/kernels/claim_set_build.hpp"

extern "C" {
int match_set_stub_calls = 0;                 // jg_claims_match_set calls so far
int match_set_stub_refused = 0;               // ... that returned -1
int match_set_stub_nsets = 0;                 // the sets the last call named
int set_stub_loads = 0;                       // successful jg_set_load calls so far
int set_stub_frees = 0;                       // successful jg_set_free calls so far
int set_stub_fail = 0;                        // != 0: jg_set_load returns -2
uint32_t set_stub_last_seed = 0;              // the seed of the last successful load
}

namespace {
struct StubSet {
  jgset::Built built;
  uint64_t generation = 0;
};
std::shared_ptr<StubSet> g_sets[JG_MAX_LOADED_SETS];
uint64_t g_generation = 0;

struct StubSetArgs : StubHashArgs {
  const uint8_t* seg;
  uint32_t seg_len;
  uint32_t peek(uint32_t g) const {
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4; ++k)
      if (4 * g + k < seg_len) w |= (uint32_t)seg[4 * g + k] << (8 * k);
    return w;
  }
};
}  // namespace

extern "C" int jg_set_load(jg_ctx*, uint32_t id, const uint8_t* bytes, size_t bytes_len, const jg_sarg* members, size_t n,
                           uint32_t seed) {
  if (id >= JG_MAX_LOADED_SETS || (n && !members)) return -1;
  if (set_stub_fail) return -2;
  auto s = std::make_shared<StubSet>();
  size_t bad = 0;
  if (jgset::set_build(bytes, bytes_len, members, n, seed, &s->built, &bad) != 0) return -1;
  s->generation = ++g_generation;
  g_sets[id] = s;
  ++set_stub_loads;
  set_stub_last_seed = seed;
  return 0;
}

extern "C" int jg_set_free(jg_ctx*, uint32_t id) {
  if (id >= JG_MAX_LOADED_SETS || !g_sets[id]) return -1;
  g_sets[id].reset();
  ++set_stub_frees;
  return 0;
}

extern "C" int jg_set_info(jg_ctx*, uint32_t id, jg_setinfo* out) {
  if (id >= JG_MAX_LOADED_SETS || !g_sets[id] || !out) return -1;
  const jgset::Built& b = g_sets[id]->built;
  *out = jg_setinfo{b.n, (uint32_t)b.slots.size(), b.maxprobe, b.seed, 4 * (uint64_t)b.pool.size(), g_sets[id]->generation};
  return 0;
}

extern "C" int jg_claims_match_set(jg_ctx*, const uint8_t* arena, size_t arena_len, const jg_cjob* jobs, size_t njobs,
                                   const jg_expect* expects, uint32_t nexpect, const jg_paths* paths, const jg_preds* preds,
                                   const jg_args* args, const jg_hargs* hargs, const jg_setargs* sets, uint8_t* code_out,
                                   uint32_t* match_out) {
  ++match_set_stub_calls;
  const auto refuse = [] { ++match_set_stub_refused; return -1; };
  if (!expects || (njobs > 0 && (!jobs || !code_out || !paths || !preds || !match_out))) return refuse();
  if (njobs == 0) return 0;
  const uint32_t ns = args ? args->nstr : 0u, nn = args ? args->nnum : 0u, nh = hargs ? hargs->nhash : 0u;
  const uint32_t nsets = sets ? sets->nsets : 0u;
  match_set_stub_nsets = (int)nsets;
  if (nsets > JG_MAX_SETS) return refuse();
  std::shared_ptr<StubSet> held[JG_MAX_SETS];
  for (uint32_t x = 0; x < nsets; ++x) {
    if (sets->id[x] >= JG_MAX_LOADED_SETS || !g_sets[sets->id[x]]) return refuse();
    held[x] = g_sets[sets->id[x]];
  }
  auto T = std::make_unique<jgclaims::Profiles>();
  auto P = std::make_unique<jgclaims::Paths>();
  auto Q = std::make_unique<jgclaims::SetArgPreds>();
  if (!jgclaims::resolve_profiles(expects, nexpect, T.get())) return refuse();
  if (!jgclaims::resolve_paths(*paths, P.get())) return refuse();
  if (!jgclaims::resolve_arg_preds(*preds, *P, ns, nn, Q.get(), true, nh, nsets, &Q->sets)) return refuse();
  for (uint32_t x = 0; x < nsets; ++x) {
    const jgset::View v = held[x]->built.view();
    Q->sets.h[x] = jgclaims::SetHeader{(uint64_t)(uintptr_t)v.slots, (uint64_t)(uintptr_t)v.pool, v.mask, v.maxprobe, v.seed, v.n};
  }
  for (size_t i = 0; i < njobs; ++i) {
    if (jobs[i].flags >= nexpect || jobs[i].off > arena_len || jobs[i].len > arena_len - jobs[i].off) return refuse();
    if (args && !jgclaims::arg_operands_ok(*args, i)) return refuse();
    if (nh && !jgclaims::hash_sources_ok(*hargs, i)) return refuse();
  }
  std::vector<std::vector<uint8_t>> hashed(njobs * nh);
  if (nh) {
    const std::vector<uint32_t> buf = padded(hargs->bytes, hargs->bytes_len);
    for (size_t t = 0; t < njobs * nh; ++t) {
      const jg_hsrc& s = hargs->src[t];
      uint32_t w[jghop::kWords];
      const uint32_t n = jghop::hash_operand((const uint8_t*)buf.data(), s.off, s.len, s.fam, w);
      for (uint32_t k = 0; k < n; ++k) hashed[t].push_back((uint8_t)(w[k >> 2] >> (8u * (k & 3u))));
    }
  }
  for (size_t i = 0; i < njobs; ++i) {
    ByteSrc src{arena + jobs[i].off, jobs[i].len};
    const StubSetArgs A{{args, &hashed, ns, nh, i}, arena + jobs[i].off, jobs[i].len};
    code_out[i] = jgclaims::claims_match_set(src, src.len, *T, jobs[i].flags, *P, *Q, A, &match_out[i]);
  }
  return 0;
}
