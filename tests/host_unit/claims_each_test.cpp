// Stand-alone host build of the per-profile registered-claims scan
// (kernels/claims.hpp resolve_profiles, claims_decide_each, claims_extract_each,
// claims_select_each): the functions the k_claims_*_each kernels run, compiled
// for the CPU.
//
//   claims_each_test CASES LO HI [NAME...]
//
// CASES is the text file of claims_scan_test.cpp, one record per line, byte
// strings in hex ("-" = empty):
//   E iss sub jti naud aud... now_sec now_nsec skew_ns exp_leeway_s nbf_leeway_s
//   C <index of an E line> <payload segment>
// The E lines [LO, HI) become one Profiles table, in order (HI may lie past the
// last E line: the table then ends there).  A table resolve_profiles() refuses,
// or a name list resolve_select() refuses, ends the program with "rejected" on
// stdout and exit status 3.
// For every C line whose E line lies in [LO, HI) the program prints, in order,
// one line: claims_decide_each's code; claims_extract_each's code and the 64
// bytes of its jg_claims; claims_select_each's code, its jg_claims and the 80
// bytes of its jg_selected -- all against profile (index - LO).  The records are
// poisoned before each call, so a field a function leaves unwritten shows.  The
// table lies in a heap block of exactly its size and the expected strings in
// blocks of exactly theirs, so ASan sees a read past the pool's last byte.
// tests/test_claims_each_model.py compares the output with the single-Expect
// programs' and also runs this program built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/kernels/claims.hpp"

namespace {

std::string unhex(const std::string& h) {
  if (h == "-") return "";
  std::string o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return o;
}

// the segment as the kernel sees it: four characters per word, little-endian;
// a copy of exactly the segment's bytes, so ASan sees any read past its end
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

void hex(const void* p, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t k = 0; k < n; ++k) std::printf("%02x", b[k]);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s CASES LO HI [NAME...]\n", argv[0]);
    return 2;
  }
  const size_t lo = std::strtoul(argv[2], nullptr, 10), hi = std::strtoul(argv[3], nullptr, 10);
  std::vector<uint8_t> names;
  jg_select sel{};
  sel.n = (uint32_t)(argc - 4);
  for (int k = 4; k < argc; ++k) {
    const std::string b = unhex(argv[k]);
    if (k - 4 < JG_MAX_SELECT) sel.name_len[k - 4] = (uint32_t)b.size();
    names.insert(names.end(), b.begin(), b.end());
  }
  if (names.empty()) names.push_back(0);
  sel.names = names.data();
  auto S = std::make_unique<jgclaims::Select>();
  if (!jgclaims::resolve_select(sel, S.get())) {
    std::printf("rejected\n");
    return 3;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<jg_expect> sets;
  std::vector<std::unique_ptr<uint8_t[]>> strs;      // one block of exactly its bytes per set
  std::vector<std::pair<size_t, std::string>> cases;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "E") {
      std::string iss, sub, jti, a;
      uint32_t naud = 0;
      ss >> iss >> sub >> jti >> naud;
      std::string all = unhex(iss);
      jg_expect x{};
      x.iss_len = (uint32_t)all.size();
      const std::string s2 = unhex(sub), s3 = unhex(jti);
      x.sub_len = (uint32_t)s2.size();
      x.jti_len = (uint32_t)s3.size();
      all += s2 + s3;
      x.naud = naud;
      for (uint32_t k = 0; k < naud; ++k) {
        ss >> a;
        const std::string b = unhex(a);
        if (k < JG_MAX_AUD) x.aud_len[k] = (uint32_t)b.size();
        all += b;
      }
      long long now_sec, skew, elw, nlw;
      unsigned now_nsec;
      ss >> now_sec >> now_nsec >> skew >> elw >> nlw;
      if (!ss) {
        std::fprintf(stderr, "bad E line: %s\n", line.c_str());
        return 2;
      }
      strs.emplace_back(new uint8_t[all.size() ? all.size() : 1]);
      std::memcpy(strs.back().get(), all.data(), all.size());
      x.strs = strs.back().get();
      x.now_sec = now_sec;
      x.now_nsec = now_nsec;
      x.skew_ns = skew;
      x.exp_leeway_s = elw;
      x.nbf_leeway_s = nlw;
      sets.push_back(x);
    } else if (tag == "C") {
      size_t idx = 0;
      std::string seg;
      ss >> idx >> seg;
      if (!ss || idx >= sets.size()) {
        std::fprintf(stderr, "bad C line: %s\n", line.c_str());
        return 2;
      }
      cases.emplace_back(idx, unhex(seg));
    } else {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  const size_t end = hi < sets.size() ? hi : sets.size();
  const size_t n = lo < end ? end - lo : 0;
  auto T = std::make_unique<jgclaims::Profiles>();
  std::memset(T.get(), 0xee, sizeof(jgclaims::Profiles));
  if (!jgclaims::resolve_profiles(n ? sets.data() + lo : sets.data(), (uint32_t)n, T.get())) {
    std::printf("rejected\n");
    return 3;
  }
  // the unused tail is zero, as resolve() leaves an Expect's
  for (size_t p = n; p < JG_MAX_PROFILES; ++p) {
    const uint8_t* h = (const uint8_t*)&T->h[p];
    for (size_t b = 0; b < sizeof T->h[p]; ++b)
      if (h[b]) { std::fprintf(stderr, "header %zu not zeroed\n", p); return 4; }
  }
  for (size_t b = T->pool_used; b < sizeof T->pool; ++b)
    if (T->pool[b]) { std::fprintf(stderr, "pool byte %zu not zeroed\n", b); return 4; }
  size_t ncases = 0;
  for (const auto& c : cases) {
    if (c.first < lo || c.first >= end) continue;
    const uint32_t p = (uint32_t)(c.first - lo);
    std::vector<uint8_t> copy(c.second.begin(), c.second.end());
    jg_claims v;
    jg_selected q;
    {
      ByteSrc src{copy.data(), (uint32_t)copy.size()};
      std::printf("%d ", (int)jgclaims::claims_decide_each(src, src.len, *T, p));
    }
    {
      ByteSrc src{copy.data(), (uint32_t)copy.size()};
      std::memset(&v, 0xee, sizeof v);
      std::printf("%d ", (int)jgclaims::claims_extract_each(src, src.len, *T, p, &v));
      hex(&v, sizeof v);
    }
    {
      ByteSrc src{copy.data(), (uint32_t)copy.size()};
      std::memset(&v, 0xee, sizeof v);
      std::memset(&q, 0xee, sizeof q);
      std::printf(" %d ", (int)jgclaims::claims_select_each(src, src.len, *T, p, *S, &v, &q));
      hex(&v, sizeof v);
      std::printf(" ");
      hex(&q, sizeof q);
    }
    std::printf("\n");
    ++ncases;
  }
  std::fprintf(stderr, "claims each: %zu profiles, %u pool bytes, %zu cases\n", n, T->pool_used, ncases);
  return 0;
}
