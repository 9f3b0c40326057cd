// Stand-alone host build of the predicate-matching registered-claims scan
// (kernels/claims.hpp claims_match_each): the function k_claims_match_each runs,
// compiled for the CPU.
//
//   claims_match_test CASES [PATH...] [-- PRED...]
//
// CASES is the text file of claims_scan_test.cpp (tests/claims_corpus.py and
// tests/claims_extract_cases.py write it), one record per line, byte strings in
// hex ("-" = empty):
//   E iss sub jti naud aud... now_sec now_nsec skew_ns exp_leeway_s nbf_leeway_s
//   C <index of an E line> <payload segment>
// PATH...: the caller's paths as claims_paths_test.cpp takes them, each its
// components in hex joined by "/" ("-" = the empty component, "@" = a path of no
// components).  PRED...: the predicates, each "<path index>:<op>:<value in hex>"
// with op the number of a jg_pred_op (any number is passed on as it is).  A list
// resolve_paths() or resolve_preds() rejects ends the program with "rejected
// paths" or "rejected preds" on stdout and exit status 3, before CASES is read.
// Every E line becomes profile 1 of a table of two (profile 0 is the file's
// first E line), so the scan reads its expected side at an offset into the pool.
// For every C line the program prints the jg_claim_code and the mask of the
// predicates that hold, in hex, one case per line, in order.  The mask is
// poisoned before the call, so a path that leaves it unwritten shows.
// tests/test_claims_match_model.py checks the output and also runs this program
// built with -fsanitize=address,undefined.
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

struct ExpectLine {
  jg_expect x{};
  std::string strs;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s CASES [PATH...] [-- PRED...]\n", argv[0]);
    return 2;
  }
  int sep = argc;
  for (int k = 2; k < argc; ++k)
    if (std::string(argv[k]) == "--") { sep = k; break; }
  // the paths as the ABI takes them: a copy of exactly their bytes
  std::vector<uint8_t> names;
  jg_paths paths{};
  paths.n = (uint32_t)(sep - 2);
  for (int k = 2; k < sep; ++k) {
    const std::string arg = argv[k];
    uint32_t nc = 0;
    if (arg != "@") {
      std::istringstream cs(arg);
      std::string comp;
      while (std::getline(cs, comp, '/')) {
        const std::string b = unhex(comp);
        if (k - 2 < JG_MAX_PATHS && nc < JG_PATH_MAX_COMP) {
          paths.comp_len[k - 2][nc] = (uint32_t)b.size();
          names.insert(names.end(), b.begin(), b.end());
        }
        ++nc;
      }
    }
    if (k - 2 < JG_MAX_PATHS) paths.ncomp[k - 2] = nc;
  }
  if (names.empty()) names.push_back(0);
  paths.names = names.data();
  auto P = std::make_unique<jgclaims::Paths>();
  if (!jgclaims::resolve_paths(paths, P.get())) {
    std::printf("rejected paths\n");
    return 3;
  }
  // the predicates likewise; past JG_MAX_PRED nothing is stored: the list is refused on its count
  std::vector<uint8_t> values;
  jg_preds preds{};
  preds.n = sep < argc ? (uint32_t)(argc - sep - 1) : 0u;
  for (int k = sep + 1; k < argc; ++k) {
    const int i = k - sep - 1;
    unsigned path = 0, op = 0;
    char hex[1024] = "";
    if (std::sscanf(argv[k], "%u:%u:%1023s", &path, &op, hex) != 3) {
      std::fprintf(stderr, "bad predicate: %s\n", argv[k]);
      return 2;
    }
    if (i >= JG_MAX_PRED) continue;
    const std::string b = unhex(hex);
    preds.path[i] = (uint8_t)path;
    preds.op[i] = (uint8_t)op;
    preds.value_len[i] = (uint32_t)b.size();
    values.insert(values.end(), b.begin(), b.end());
  }
  std::vector<uint8_t> vcopy(values);                 // exactly the values' bytes; NULL when there are none
  preds.values = vcopy.empty() ? nullptr : vcopy.data();
  auto Q = std::make_unique<jgclaims::Preds>();
  if (!jgclaims::resolve_preds(preds, *P, Q.get())) {
    std::printf("rejected preds\n");
    return 3;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<std::unique_ptr<ExpectLine>> lines;
  std::vector<std::unique_ptr<jgclaims::Profiles>> tables;
  std::string line;
  size_t ncases = 0;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "E") {
      std::string iss, sub, jti, a;
      uint32_t naud = 0;
      ss >> iss >> sub >> jti >> naud;
      auto L = std::make_unique<ExpectLine>();
      jg_expect& x = L->x;
      L->strs = unhex(iss);
      x.iss_len = (uint32_t)L->strs.size();
      const std::string s2 = unhex(sub), s3 = unhex(jti);
      x.sub_len = (uint32_t)s2.size();
      x.jti_len = (uint32_t)s3.size();
      L->strs += s2 + s3;
      x.naud = naud;
      for (uint32_t k = 0; k < naud; ++k) {
        ss >> a;
        const std::string b = unhex(a);
        if (k < JG_MAX_AUD) x.aud_len[k] = (uint32_t)b.size();
        L->strs += b;
      }
      long long now_sec, skew, elw, nlw;
      unsigned now_nsec;
      ss >> now_sec >> now_nsec >> skew >> elw >> nlw;
      if (!ss) {
        std::fprintf(stderr, "bad E line: %s\n", line.c_str());
        return 2;
      }
      x.strs = (const uint8_t*)L->strs.data();
      x.now_sec = now_sec;
      x.now_nsec = now_nsec;
      x.skew_ns = skew;
      x.exp_leeway_s = elw;
      x.nbf_leeway_s = nlw;
      lines.push_back(std::move(L));
      const jg_expect two[2] = {lines.front()->x, lines.back()->x};
      auto T = std::make_unique<jgclaims::Profiles>();
      if (!jgclaims::resolve_profiles(two, 2, T.get())) {
        std::fprintf(stderr, "expected set rejected: %s\n", line.c_str());
        return 2;
      }
      tables.push_back(std::move(T));
    } else if (tag == "C") {
      size_t idx = 0;
      std::string seg;
      ss >> idx >> seg;
      if (!ss || idx >= tables.size()) {
        std::fprintf(stderr, "bad C line: %s\n", line.c_str());
        return 2;
      }
      const std::string b = unhex(seg);
      std::vector<uint8_t> copy(b.begin(), b.end());
      ByteSrc src{copy.data(), (uint32_t)copy.size()};
      uint32_t mask = 0xeeeeeeeeu;
      const int code = (int)jgclaims::claims_match_each(src, src.len, *tables[idx], 1u, *P, *Q, &mask);
      std::printf("%d %08x\n", code, mask);
      ++ncases;
    } else {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  std::fprintf(stderr, "claims match: %zu cases\n", ncases);
  return 0;
}
