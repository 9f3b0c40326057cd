// match_hash_stub.cpp -- tests/host_match_args/match_args_stub.cpp (a stand-in
// for libcapjwt.so's C ABI whose verify accepts every job and whose claims scans
// run the CPU build of the device's functions) plus jg_claims_match_hash, which
// runs the CPU build of resolve_arg_preds with the hash ops, hash_sources_ok,
// hash_operand (kernels/hash_operand.hpp, through tests/host_kernels' stand-in
// for the HIP header) and claims_match_args, and refuses what the ABI refuses;
// and a jg_hash_batch that hashes (the chain's own always fails), with a switch
// to make it fail.  For the host layer of the MatchArgs entries with hash
// columns without a GPU (match_hash.cpp, tests/test_host_match_hash.py).
#define jg_hash_batch chain_hash_batch_that_fails
#include "../host_match_args/match_args_stub.cpp"
#undef jg_hash_batch

#include <vector>

#include "../../cap_amd/csrc/kernels/hash_operand.hpp"

extern "C" {
int match_hash_stub_calls = 0;                // jg_claims_match_hash calls so far
int match_hash_stub_refused = 0;              // ... that returned -1
int match_hash_stub_sources = 0;              // sources with a family the last call hashed
int hash_stub_calls = 0;                      // jg_hash_batch calls so far
int hash_stub_jobs = 0;                       // ... and the jobs of the last one
int hash_stub_fail = 0;                       // != 0: jg_hash_batch returns -2
}

namespace {
// a copy of the bytes with the slack the runtime gives its device buffers, word-aligned
std::vector<uint32_t> padded(const uint8_t* p, size_t n) {
  std::vector<uint32_t> buf((n + 3) / 4 + 64, 0u);
  if (n) std::memcpy(buf.data(), p, n);
  return buf;
}

struct StubHashArgs {
  const jg_args* a;                           // may be NULL
  const std::vector<std::vector<uint8_t>>* hashed;   // njobs x nhash operands
  uint32_t ns, nh;
  size_t i;
  uint32_t nstr() const { return ns + nh; }
  const uint8_t* bytes(uint32_t c, uint32_t* l) const {
    if (c < ns) {
      const jg_sarg& s = a->str[i * ns + c];
      *l = s.len;
      return a->bytes + s.off;
    }
    const std::vector<uint8_t>& v = (*hashed)[i * nh + (c - ns)];
    *l = (uint32_t)v.size();
    return v.data();
  }
  uint32_t slen(uint32_t c) const {
    uint32_t l;
    (void)bytes(c, &l);
    return l;
  }
  uint32_t word(uint32_t c, uint32_t p) const {
    uint32_t l;
    const uint8_t* b = bytes(c, &l);
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4; ++k)
      if (p + k < l) w |= (uint32_t)b[p + k] << (8 * k);
    return w;
  }
  int64_t bound(uint32_t c) const { return a->num[i * a->nnum + c]; }
};
}  // namespace

extern "C" int jg_hash_batch(jg_ctx*, const uint8_t* arena, size_t arena_len, const jg_hjob* jobs, size_t njobs,
                             uint8_t* digest_out) {
  ++hash_stub_calls;
  hash_stub_jobs = (int)njobs;
  if (hash_stub_fail) return -2;
  const std::vector<uint32_t> buf = padded(arena, arena_len);
  for (size_t i = 0; i < njobs; ++i) {
    const jg_hjob& J = jobs[i];
    if (J.fam < JG_SHA256 || J.fam > JG_SHA512 || J.off > arena_len || J.len > arena_len - J.off) return -1;
    sha2::MemString m{buf.data() + (J.off >> 2), (uint32_t)(J.off & 3), J.len};
    uint8_t* o = digest_out + 64 * i;
    std::memset(o, 0, 64);
    if (J.fam == JG_SHA256) {
      uint32_t h[8];
      sha2::sha256_mem(h, m);
      for (int k = 0; k < 8; ++k)
        for (int b = 0; b < 4; ++b) o[4 * k + b] = (uint8_t)(h[k] >> (24 - 8 * b));
    } else {
      uint64_t h[8];
      sha2::sha512_mem(h, J.fam == JG_SHA384, m, nullptr, 0);
      for (int k = 0; k < 8; ++k)
        for (int b = 0; b < 8; ++b) o[8 * k + b] = (uint8_t)(h[k] >> (56 - 8 * b));
    }
  }
  return 0;
}

extern "C" int jg_claims_match_hash(jg_ctx*, const uint8_t* arena, size_t arena_len, const jg_cjob* jobs, size_t njobs,
                                    const jg_expect* expects, uint32_t nexpect, const jg_paths* paths,
                                    const jg_preds* preds, const jg_args* args, const jg_hargs* hargs, uint8_t* code_out,
                                    uint32_t* match_out) {
  ++match_hash_stub_calls;
  const auto refuse = [] { ++match_hash_stub_refused; return -1; };
  if (!expects || (njobs > 0 && (!jobs || !code_out || !paths || !preds || !match_out))) return refuse();
  if (njobs == 0) return 0;
  const uint32_t ns = args ? args->nstr : 0u, nn = args ? args->nnum : 0u, nh = hargs ? hargs->nhash : 0u;
  auto T = std::make_unique<jgclaims::Profiles>();
  auto P = std::make_unique<jgclaims::Paths>();
  auto Q = std::make_unique<jgclaims::ArgPreds>();
  if (!jgclaims::resolve_profiles(expects, nexpect, T.get())) return refuse();
  if (!jgclaims::resolve_paths(*paths, P.get())) return refuse();
  if (!jgclaims::resolve_arg_preds(*preds, *P, ns, nn, Q.get(), true, nh)) return refuse();
  if (args && ((args->bytes_len && !args->bytes) || (ns && !args->str) || (nn && !args->num))) return refuse();
  if (hargs && ((hargs->bytes_len && !hargs->bytes) || (nh && !hargs->src))) return refuse();
  for (size_t i = 0; i < njobs; ++i) {
    if (jobs[i].flags >= nexpect || jobs[i].off > arena_len || jobs[i].len > arena_len - jobs[i].off) return refuse();
    if (args && !jgclaims::arg_operands_ok(*args, i)) return refuse();
    if (nh && !jgclaims::hash_sources_ok(*hargs, i)) return refuse();
  }
  std::vector<std::vector<uint8_t>> hashed(njobs * nh);
  match_hash_stub_sources = 0;
  if (nh) {
    const std::vector<uint32_t> buf = padded(hargs->bytes, hargs->bytes_len);
    for (size_t t = 0; t < njobs * nh; ++t) {
      const jg_hsrc& s = hargs->src[t];
      uint32_t w[jghop::kWords];
      const uint32_t n = jghop::hash_operand((const uint8_t*)buf.data(), s.off, s.len, s.fam, w);
      for (uint32_t k = 0; k < n; ++k) hashed[t].push_back((uint8_t)(w[k >> 2] >> (8u * (k & 3u))));
      match_hash_stub_sources += s.fam != 0;
    }
  }
  for (size_t i = 0; i < njobs; ++i) {
    ByteSrc src{arena + jobs[i].off, jobs[i].len};
    const StubHashArgs A{args, &hashed, ns, nh, i};
    code_out[i] = jgclaims::claims_match_args(src, src.len, *T, jobs[i].flags, *P, *Q, A, &match_out[i]);
  }
  return 0;
}
