// Stand-alone host build of what jg_claims_match_set runs on the device: the
// predicate-matching claims scan with set predicates (kernels/claims.hpp
// claims_match_set, resolved with the hash and the set ops switched on) against
// sets built by kernels/claim_set.hpp set_build(), compiled for the CPU with
// tests/host_kernels' stand-in for the HIP header.
//
//   claims_match_set_test CASES ARGS SETS [PATH...] [-- PRED...]
//
// CASES, ARGS, PATH and PRED are claims_match_hash_test's, with two more ops --
// 12 (IN_SET) and 13 (ELEMENT_IN_SET): the value is one byte, the set index.
// SETS is "-" (no set) or a file with one line per set of the call, in order:
//   S <seed> [<member in hex, "-" = empty>...]
// A list resolve_paths() or resolve_arg_preds() rejects ends the program with
// "rejected paths" or "rejected preds", more than JG_MAX_SETS sets or a set
// set_build() refuses with "rejected sets", operands and sources as
// claims_match_hash_test says, on stdout and exit status 3.  For every C line the
// program prints the jg_claim_code and the mask.  A list without a set op is
// scanned by claims_match_args, as the runtime launches that kernel for it: with
// ops 1..11 the program prints what claims_match_hash_test prints.
// tests/test_claims_match_set_model.py checks the output and also runs this
// program built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/kernels/claim_set_build.hpp"
#include "../../cap_amd/csrc/kernels/claims.hpp"
#include "../../cap_amd/csrc/kernels/hash_operand.hpp"

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

// one hashed operand: hash_operand()'s words as exactly its bytes
struct Hashed {
  std::vector<uint8_t> bytes;
};

// the operand of src[off, off + len) under fam.  The hash reads aligned words around the source: the copy
// has the slack the runtime gives the device buffer (256 zero bytes) and is word-aligned.
Hashed make_operand(const uint8_t* src, uint32_t off, uint32_t len, uint32_t fam, size_t total) {
  std::vector<uint32_t> buf((total + 3) / 4 + 64, 0u);
  if (total) std::memcpy(buf.data(), src, total);
  uint32_t w[jghop::kWords];
  const uint32_t n = jghop::hash_operand((const uint8_t*)buf.data(), off, len, fam, w);
  Hashed h;
  for (uint32_t k = 0; k < n; ++k) h.bytes.push_back((uint8_t)(w[k >> 2] >> (8u * (k & 3u))));
  for (uint32_t k = n; k < 4u * jghop::kWords; ++k)
    if ((w[k >> 2] >> (8u * (k & 3u))) & 0xffu) std::abort();       // zero behind the last character
  return h;
}

// job i's operands as the scan reads them: the caller's columns, then the hashed ones
struct HostArgs {
  const jg_args* a;
  const std::vector<Hashed>* hashed;   // njobs x nhash
  uint32_t nhash;
  size_t i;
  uint32_t nstr() const { return a->nstr + nhash; }
  uint32_t slen(uint32_t c) const {
    return c < a->nstr ? a->str[i * a->nstr + c].len : (uint32_t)(*hashed)[i * nhash + (c - a->nstr)].bytes.size();
  }
  uint32_t word(uint32_t c, uint32_t p) const {
    const uint32_t l = slen(c);
    if (p >= l || (p & 3u)) std::abort();              // the scan asks only for a window it needs
    const uint8_t* b = c < a->nstr ? a->bytes + a->str[i * a->nstr + c].off : (*hashed)[i * nhash + (c - a->nstr)].bytes.data();
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4; ++k)
      if (p + k < l) w |= (uint32_t)b[p + k] << (8 * k);
    return w;
  }
  int64_t bound(uint32_t c) const { return a->num[i * a->nnum + c]; }
};

// HostArgs and the segment again, group by group in any order
struct HostSetArgs : HostArgs {
  const uint8_t* seg;
  uint32_t seg_len;
  uint32_t ngroups;                    // the groups the scan may have read
  uint32_t peek(uint32_t g) const {
    if (g >= ngroups) std::abort();
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4; ++k)
      if (4 * g + k < seg_len) w |= (uint32_t)seg[4 * g + k] << (8 * k);
    return w;
  }
};

struct ExpectLine {
  jg_expect x{};
  std::string strs;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s CASES ARGS SETS [PATH...] [-- PRED...]\n", argv[0]);
    return 2;
  }
  const int first = 4;
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
  // the operands and the hash sources: the bytes back to back, a copy of exactly them
  std::vector<uint8_t> abytes, hbytes;
  std::vector<jg_sarg> astr;
  std::vector<int64_t> anum;
  std::vector<jg_hsrc> hsrc;
  jg_args args{};
  jg_hargs hargs{};
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
        if (ss && !(ss >> hargs.nhash)) {
          hargs.nhash = 0;
          ss.clear();
        }
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
        for (uint32_t c = 0; c < hargs.nhash; ++c) {
          std::string h;
          ss >> h;
          const size_t colon = h.find(':');
          if (!ss || colon == std::string::npos) {
            ss.setstate(std::ios::failbit);
            break;
          }
          const std::string b = unhex(h.substr(colon + 1));
          jg_hsrc s{};
          s.off = (uint32_t)hbytes.size();
          s.len = (uint32_t)b.size();
          s.fam = (uint8_t)std::stoi(h.substr(0, colon));
          hsrc.push_back(s);
          hbytes.insert(hbytes.end(), b.begin(), b.end());
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
  std::vector<uint8_t> acopy(abytes), hcopy(hbytes);
  args.bytes = acopy.empty() ? nullptr : acopy.data();
  args.bytes_len = acopy.size();
  args.str = astr.empty() ? nullptr : astr.data();
  args.num = anum.empty() ? nullptr : anum.data();
  hargs.bytes = hcopy.empty() ? nullptr : hcopy.data();
  hargs.bytes_len = hcopy.size();
  hargs.src = hsrc.empty() ? nullptr : hsrc.data();
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
  // the sets of the call
  std::vector<jgset::Built> built;
  if (std::string(argv[3]) != "-") {
    std::ifstream sin(argv[3]);
    if (!sin) {
      std::fprintf(stderr, "cannot open %s\n", argv[3]);
      return 2;
    }
    std::string line, tag, tok;
    while (std::getline(sin, line)) {
      if (line.empty()) continue;
      std::istringstream ss(line);
      unsigned long seed = 0;
      ss >> tag >> seed;
      if (!ss || tag != "S") {
        std::fprintf(stderr, "bad set line: %s\n", line.c_str());
        return 2;
      }
      std::vector<uint8_t> bytes;
      std::vector<jg_sarg> members;
      while (ss >> tok) {
        const std::string b = unhex(tok);
        members.push_back(jg_sarg{(uint32_t)bytes.size(), (uint32_t)b.size()});
        bytes.insert(bytes.end(), b.begin(), b.end());
      }
      std::vector<uint8_t> copy(bytes);
      built.emplace_back();
      if (jgset::set_build(copy.empty() ? nullptr : copy.data(), copy.size(), members.empty() ? nullptr : members.data(),
                           members.size(), (uint32_t)seed, &built.back(), nullptr) != 0) {
        std::printf("rejected sets\n");
        return 3;
      }
    }
  }
  if (built.size() > JG_MAX_SETS) {
    std::printf("rejected sets\n");
    return 3;
  }
  auto Q = std::make_unique<jgclaims::SetArgPreds>();
  if (!jgclaims::resolve_arg_preds(preds, *P, args.nstr, args.nnum, Q.get(), true, hargs.nhash, (uint32_t)built.size(),
                                   &Q->sets)) {
    std::printf("rejected preds\n");
    return 3;
  }
  bool setop = false;
  for (uint32_t k = 0; k < JG_MAX_PATHS; ++k) setop = setop || Q->sets.inset[k] || Q->sets.elemset[k];
  for (size_t x = 0; x < built.size(); ++x) {
    const jgset::View v = built[x].view();
    Q->sets.h[x] = jgclaims::SetHeader{(uint64_t)(uintptr_t)v.slots, (uint64_t)(uintptr_t)v.pool, v.mask, v.maxprobe, v.seed, v.n};
  }
  const size_t nops = args.nstr ? astr.size() / args.nstr : args.nnum ? anum.size() / args.nnum
                      : hargs.nhash ? hsrc.size() / hargs.nhash : 0;
  std::vector<Hashed> hashed;
  for (size_t i = 0; i < nops; ++i) {
    if (!jgclaims::arg_operands_ok(args, i)) {
      std::printf("rejected args %zu\n", i);
      return 3;
    }
    if (!jgclaims::hash_sources_ok(hargs, i)) {
      std::printf("rejected hsrc %zu\n", i);
      return 3;
    }
    for (uint32_t c = 0; c < hargs.nhash; ++c) {
      const jg_hsrc& s = hargs.src[i * hargs.nhash + c];
      hashed.push_back(make_operand(hargs.bytes, s.off, s.len, s.fam, hargs.bytes_len));
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
      if ((args.nstr || args.nnum || hargs.nhash) && ncases >= nops) {
        std::fprintf(stderr, "no operands for case %zu\n", ncases);
        return 2;
      }
      const std::string b = unhex(seg);
      std::vector<uint8_t> copy(b.begin(), b.end());
      ByteSrc src{copy.data(), (uint32_t)copy.size()};
      const HostSetArgs A{{&args, &hashed, hargs.nhash, ncases}, copy.data(), src.len, (src.len + 3u) / 4u};
      uint32_t mask = 0xeeeeeeeeu;
      const int code = setop ? (int)jgclaims::claims_match_set(src, src.len, *tables[idx], 1u, *P, *Q, A, &mask)
                             : (int)jgclaims::claims_match_args(src, src.len, *tables[idx], 1u, *P, *Q, A, &mask);
      std::printf("%d %08x\n", code, mask);
      ++ncases;
    } else {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  std::fprintf(stderr, "claims match set: %zu cases\n", ncases);
  return 0;
}
