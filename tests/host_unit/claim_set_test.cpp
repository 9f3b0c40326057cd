// Stand-alone host build of kernels/claim_set_build.hpp and claim_set.hpp: set_build() and set_probe()
// for the CPU, so tests/test_set_model.py can compare the table byte for byte
// with its plain-Python model and every lookup with Python's `in`.
//
//   claim_set_test FILE
//
// FILE holds lines
//   B <seed> [<member in hex, "-" = empty>...]    build a set; prints
//        "T <n> <nslots> <maxprobe> <slots in hex> <pool in hex, "-" = empty>"
//        (both little-endian, as they are uploaded), or "rejected <member index>",
//        after which queries are answered against no set at all
//   Q <query in hex, "-" = empty>                 prints "1" or "0": set_probe on the last set built
// The members are handed to set_build() as exactly their bytes back to back and
// a query's bytes as exactly its own, so ASan sees any read past either.
// tests/test_set_model.py also runs this program built with
// -fsanitize=address,undefined.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/kernels/claim_set_build.hpp"

namespace {

std::string unhex(const std::string& h) {
  if (h == "-") return "";
  std::string o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return o;
}

void put_words(const uint32_t* w, size_t n) {
  if (n == 0) std::printf("-");
  for (size_t k = 0; k < n; ++k)
    std::printf("%02x%02x%02x%02x", w[k] & 0xffu, (w[k] >> 8) & 0xffu, (w[k] >> 16) & 0xffu, w[k] >> 24);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s FILE\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  jgset::Built B;
  bool have = false;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    std::string tag, tok;
    ss >> tag;
    if (tag == "B") {
      unsigned long seed = 0;
      ss >> seed;
      std::vector<uint8_t> bytes;
      std::vector<jg_sarg> members;
      while (ss >> tok) {
        const std::string b = unhex(tok);
        members.push_back(jg_sarg{(uint32_t)bytes.size(), (uint32_t)b.size()});
        bytes.insert(bytes.end(), b.begin(), b.end());
      }
      std::vector<uint8_t> copy(bytes);                // exactly the members' bytes
      size_t bad = 0;
      B = jgset::Built{};
      const int rc = jgset::set_build(copy.empty() ? nullptr : copy.data(), copy.size(),
                                      members.empty() ? nullptr : members.data(), members.size(), (uint32_t)seed, &B, &bad);
      have = rc == 0;
      if (rc != 0) {
        std::printf("rejected %zu\n", bad);
        continue;
      }
      std::printf("T %u %zu %u ", B.n, B.slots.size(), B.maxprobe);
      put_words((const uint32_t*)B.slots.data(), 2 * B.slots.size());
      std::printf(" ");
      put_words(B.pool.data(), B.pool.size());
      std::printf("\n");
    } else if (tag == "Q") {
      ss >> tok;
      const std::string q = unhex(tok);
      std::vector<uint8_t> copy(q.begin(), q.end());
      bool hit = false;
      if (have) {
        uint32_t h = jgset::kHashBasis;
        for (uint8_t c : copy) h = jgset::set_hash_step(h, c);
        const uint8_t* p = copy.data();
        hit = jgset::set_probe(B.view(), jgset::set_hash_final(h, B.seed), (uint32_t)copy.size(),
                               [p](uint32_t i) -> uint32_t { return p[i]; });
      }
      std::printf("%d\n", hit ? 1 : 0);
    } else {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
