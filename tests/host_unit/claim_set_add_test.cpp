// Stand-alone host build of kernels/claim_set_insert.hpp: the insertion and the
// rehash step for the CPU with a sequential compare-and-swap, so
// tests/test_set_add_model.py can hold what they make against
// tests/set_add_model.py's checker and every lookup against Python's `in`.
//
//   claim_set_add_test FILE
//
// FILE holds lines
//   B <seed> [<member in hex, "-" = empty>...]    build a set with set_build(); prints
//        "T <n> <nslots> <maxprobe> <slots in hex> <pool in hex, "-" = empty>"
//   A [<member in hex>...]                        add to the last set built; prints the
//        same line with " <added>" behind it, or "rejected <member index>", after
//        which the set is what it was
//   Q <query in hex, "-" = empty>                 prints "1" or "0": set_probe on the set
// The members are handed over as exactly their bytes back to back, so ASan sees
// any read past them.  tests/test_set_add_model.py also runs this program built
// with -fsanitize=address,undefined.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "claim_set_add_cpu.hpp"

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

void put_table(const jgset::Built& B) {
  std::printf("T %u %zu %u ", B.n, B.slots.size(), B.maxprobe);
  put_words((const uint32_t*)B.slots.data(), 2 * B.slots.size());
  std::printf(" ");
  put_words(B.pool.data(), B.pool.size());
}

void read_members(std::istringstream& ss, std::vector<uint8_t>* bytes, std::vector<jg_sarg>* members) {
  std::string tok;
  while (ss >> tok) {
    const std::string b = unhex(tok);
    members->push_back(jg_sarg{(uint32_t)bytes->size(), (uint32_t)b.size()});
    bytes->insert(bytes->end(), b.begin(), b.end());
  }
  bytes->shrink_to_fit();
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
  B.slots.assign(1, jgset::Slot{0u, 0u});
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    std::string tag, tok;
    ss >> tag;
    if (tag == "B" || tag == "A") {
      unsigned long seed = 0;
      if (tag == "B") ss >> seed;
      std::vector<uint8_t> bytes;
      std::vector<jg_sarg> members;
      read_members(ss, &bytes, &members);
      const std::vector<uint8_t> copy(bytes.begin(), bytes.end());   // exactly the members' bytes
      const uint8_t* p = copy.empty() ? nullptr : copy.data();
      const jg_sarg* m = members.empty() ? nullptr : members.data();
      size_t bad = 0;
      uint32_t added = 0;
      int rc;
      if (tag == "B") {
        B = jgset::Built{};
        rc = jgset::set_build(p, copy.size(), m, members.size(), (uint32_t)seed, &B, &bad);
        if (rc != 0) {
          std::fprintf(stderr, "B: member %zu refused\n", bad);
          return 2;
        }
      } else {
        rc = jgset::set_add_cpu(&B, p, copy.size(), m, members.size(), &added, &bad);
        if (rc == -1) {
          std::printf("rejected %zu\n", bad);
          continue;
        }
        if (rc != 0) {
          std::fprintf(stderr, "A: set_add_cpu returned %d\n", rc);
          return 2;
        }
      }
      put_table(B);
      if (tag == "A") std::printf(" %u", added);
      std::printf("\n");
    } else if (tag == "Q") {
      ss >> tok;
      const std::string q = unhex(tok);
      std::vector<uint8_t> copy(q.begin(), q.end());
      uint32_t h = jgset::kHashBasis;
      for (uint8_t c : copy) h = jgset::set_hash_step(h, c);
      const uint8_t* p = copy.data();
      const bool hit = jgset::set_probe(B.view(), jgset::set_hash_final(h, B.seed), (uint32_t)copy.size(),
                                        [p](uint32_t i) -> uint32_t { return p[i]; });
      std::printf("%d\n", hit ? 1 : 0);
    } else {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
