// Stand-alone host build of the predicate-matching claims scan with per-token
// operands and numeric tests (kernels/claims.hpp claims_match_args): the function
// k_claims_match_args runs, compiled for the CPU.
//
//   claims_match_args_test CASES ARGS [PATH...] [-- PRED...]
//
// CASES, PATH... and PRED... are claims_match_test.cpp's: the text file of E and
// C lines, the paths in hex joined by "/", the predicates as
// "<path index>:<op>:<value in hex>".  For the ops only jg_claims_match_args
// takes, the value is what the ABI takes: one byte (the column) for op 5, 8 and
// 9, eight bytes (the bound, little-endian) for op 6 and 7.
// ARGS is the operands' text file, or "-" for no columns:
//   A <nstr> <nnum>                        once, first
//   O <nstr strings in hex, "-" = empty> <nnum decimal int64>     one per C line, in order
// A list resolve_paths() or resolve_arg_preds() rejects ends the program with
// "rejected paths" or "rejected preds", operands arg_operands_ok() rejects with
// "rejected args <job>", on stdout and exit status 3.
// For every C line the program prints the jg_claim_code and the mask, as
// claims_match_test does; with ops 1..4 only the two programs print the same.
// The operand bytes are a copy of exactly their bytes, and the window the scan
// asks for is put together byte by byte inside the operand, so ASan sees any
// read outside it.  tests/test_claims_match_args_model.py checks the output and
// also runs this program built with -fsanitize=address,undefined.
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

// job i's operands as the scan reads them
struct HostArgs {
  const jg_args* a;
  size_t i;
  uint32_t nstr() const { return a->nstr; }
  uint32_t slen(uint32_t c) const { return a->str[i * a->nstr + c].len; }
  uint32_t word(uint32_t c, uint32_t p) const {
    const jg_sarg& s = a->str[i * a->nstr + c];
    if (p >= s.len || (p & 3u)) std::abort();          // the scan asks only for a window it needs
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4; ++k)
      if (p + k < s.len) w |= (uint32_t)a->bytes[s.off + p + k] << (8 * k);
    return w;
  }
  int64_t bound(uint32_t c) const { return a->num[i * a->nnum + c]; }
};

struct ExpectLine {
  jg_expect x{};
  std::string strs;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s CASES ARGS [PATH...] [-- PRED...]\n", argv[0]);
    return 2;
  }
  const int first = 3;
  int sep = argc;
  for (int k = first; k < argc; ++k)
    if (std::string(argv[k]) == "--") { sep = k; break; }
  // the paths as the ABI takes them: a copy of exactly their bytes
  std::vector<uint8_t> names;
  jg_paths paths{};
  paths.n = (uint32_t)(sep - first);
  for (int k = first; k < sep; ++k) {
    const std::string arg = argv[k];
    const int pk = k - first;
    uint32_t nc = 0;
    if (arg != "@") {
      std::istringstream cs(arg);
      std::string comp;
      while (std::getline(cs, comp, '/')) {
        const std::string b = unhex(comp);
        if (pk < JG_MAX_PATHS && nc < JG_PATH_MAX_COMP) {
          paths.comp_len[pk][nc] = (uint32_t)b.size();
          names.insert(names.end(), b.begin(), b.end());
        }
        ++nc;
      }
    }
    if (pk < JG_MAX_PATHS) paths.ncomp[pk] = nc;
  }
  if (names.empty()) names.push_back(0);
  paths.names = names.data();
  auto P = std::make_unique<jgclaims::Paths>();
  if (!jgclaims::resolve_paths(paths, P.get())) {
    std::printf("rejected paths\n");
    return 3;
  }
  // the operands: the bytes back to back, a copy of exactly them
  std::vector<uint8_t> abytes;
  std::vector<jg_sarg> astr;
  std::vector<int64_t> anum;
  jg_args args{};
  if (std::string(argv[2]) != "-") {
    std::ifstream ain(argv[2]);
    if (!ain) {
      std::fprintf(stderr, "cannot open %s\n", argv[2]);
      return 2;
    }
    std::string line, tag;
    bool head = false;
    while (std::getline(ain, line)) {
      if (line.empty()) continue;
      std::istringstream ss(line);
      ss >> tag;
      if (tag == "A" && !head) {
        ss >> args.nstr >> args.nnum;
        head = true;
      } else if (tag == "O" && head) {
        for (uint32_t c = 0; c < args.nstr; ++c) {
          std::string h;
          ss >> h;
          const std::string b = unhex(h);
          astr.push_back(jg_sarg{(uint32_t)abytes.size(), (uint32_t)b.size()});
          abytes.insert(abytes.end(), b.begin(), b.end());
        }
        for (uint32_t c = 0; c < args.nnum; ++c) {
          long long v = 0;
          ss >> v;
          anum.push_back((int64_t)v);
        }
      } else {
        ss.setstate(std::ios::failbit);
      }
      if (!ss) {
        std::fprintf(stderr, "bad operand line: %s\n", line.c_str());
        return 2;
      }
    }
  }
  std::vector<uint8_t> acopy(abytes);
  args.bytes = acopy.empty() ? nullptr : acopy.data();
  args.bytes_len = acopy.size();
  args.str = astr.empty() ? nullptr : astr.data();
  args.num = anum.empty() ? nullptr : anum.data();
  // the predicates; past JG_MAX_PRED nothing is stored: the list is refused on its count
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
  auto Q = std::make_unique<jgclaims::ArgPreds>();
  if (!jgclaims::resolve_arg_preds(preds, *P, args.nstr, args.nnum, Q.get())) {
    std::printf("rejected preds\n");
    return 3;
  }
  const size_t nops = args.nstr ? astr.size() / args.nstr : args.nnum ? anum.size() / args.nnum : 0;
  for (size_t i = 0; i < nops; ++i) {
    if (!jgclaims::arg_operands_ok(args, i)) {
      std::printf("rejected args %zu\n", i);
      return 3;
    }
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
      if ((args.nstr || args.nnum) && ncases >= nops) {
        std::fprintf(stderr, "no operands for case %zu\n", ncases);
        return 2;
      }
      const std::string b = unhex(seg);
      std::vector<uint8_t> copy(b.begin(), b.end());
      ByteSrc src{copy.data(), (uint32_t)copy.size()};
      const HostArgs A{&args, ncases};
      uint32_t mask = 0xeeeeeeeeu;
      const int code = (int)jgclaims::claims_match_args(src, src.len, *tables[idx], 1u, *P, *Q, A, &mask);
      std::printf("%d %08x\n", code, mask);
      ++ncases;
    } else {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  std::fprintf(stderr, "claims match args: %zu cases\n", ncases);
  return 0;
}
