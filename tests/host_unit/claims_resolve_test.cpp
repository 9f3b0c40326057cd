// Stand-alone host program for the resolvers of kernels/claims.hpp: resolve(),
// resolve_profiles(), resolve_select() and resolve_paths() on a fixed list of
// inputs.  What they fill is what the claims kernels read, byte for byte.
//
//   claims_resolve_test
//
// For every input the program prints one line, "<resolver>/<case> <hex>": the
// sizeof(Expect) / sizeof(Profiles) / sizeof(Select) / sizeof(Paths) bytes the
// resolver filled, or "<resolver>/<case> refused" where it returns false.  The
// object is 0xaa in every byte before the call, so a byte the resolver leaves
// unwritten (Expect's tail padding) prints as aa and one it stops writing shows.
// tests/test_claims_resolve.py compares the SHA-256 of every line's bytes with
// tests/golden/claims_resolve_digests.txt and also runs this program built with
// -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/kernels/claims.hpp"

namespace {

using namespace jgclaims;

// one jg_expect and the exact bytes its strs points at (none: NULL)
struct Ex {
  jg_expect x{};
  std::vector<uint8_t> strs;
};

// string k of a case: `len` bytes that depend on k and the position
void add(Ex& e, uint32_t* len_field, uint32_t len, uint32_t salt) {
  *len_field = len;
  for (uint32_t b = 0; b < len; ++b) e.strs.push_back((uint8_t)(0x21 + (salt * 7 + b * 13) % 0x5e));
}

Ex make(uint32_t iss, uint32_t sub, uint32_t jti, const std::vector<uint32_t>& auds, int64_t now_sec = 1700000000,
        uint32_t now_nsec = 0, int64_t skew_ns = 0, int64_t exp_leeway = 0, int64_t nbf_leeway = 0) {
  Ex e;
  add(e, &e.x.iss_len, iss, 1);
  add(e, &e.x.sub_len, sub, 2);
  add(e, &e.x.jti_len, jti, 3);
  e.x.naud = (uint32_t)auds.size();
  for (size_t k = 0; k < auds.size() && k < JG_MAX_AUD; ++k) add(e, &e.x.aud_len[k], auds[k], 4 + (uint32_t)k);
  e.x.now_sec = now_sec;
  e.x.now_nsec = now_nsec;
  e.x.skew_ns = skew_ns;
  e.x.exp_leeway_s = exp_leeway;
  e.x.nbf_leeway_s = nbf_leeway;
  return e;
}

// the ABI's view: strs points at a heap copy of exactly the bytes (ASan sees a read past them)
struct Bound {
  std::vector<std::unique_ptr<uint8_t[]>> keep;
  std::vector<jg_expect> x;
  explicit Bound(const std::vector<Ex>& es, bool null_strs = false) {
    for (const Ex& e : es) {
      jg_expect v = e.x;
      v.strs = nullptr;
      if (!e.strs.empty() && !null_strs) {
        keep.emplace_back(new uint8_t[e.strs.size()]);
        std::memcpy(keep.back().get(), e.strs.data(), e.strs.size());
        v.strs = keep.back().get();
      }
      x.push_back(v);
    }
  }
};

template <class T>
void show(const char* resolver, const std::string& name, bool ok, const T& obj) {
  std::printf("%s/%s ", resolver, name.c_str());
  if (!ok) {
    std::printf("refused\n");
    return;
  }
  const uint8_t* p = (const uint8_t*)&obj;
  for (size_t b = 0; b < sizeof(T); ++b) std::printf("%02x", p[b]);
  std::printf("\n");
}

template <class T>
std::unique_ptr<T> poisoned() {
  std::unique_ptr<T> o(new T);
  std::memset((void*)o.get(), 0xaa, sizeof(T));
  return o;
}

void run_expect(const std::string& name, const Ex& e, bool null_strs = false) {
  const Bound b({e}, null_strs);
  auto E = poisoned<Expect>();
  show("resolve", name, resolve(b.x[0], E.get()), *E);
  auto T = poisoned<Profiles>();                     // the same input as a table of one
  show("resolve_profiles", "one_" + name, resolve_profiles(b.x.data(), 1, T.get()), *T);
}

void run_profiles(const std::string& name, const std::vector<Ex>& es, bool null_strs = false) {
  const Bound b(es, null_strs);
  auto T = poisoned<Profiles>();
  show("resolve_profiles", name, resolve_profiles(b.x.data(), (uint32_t)b.x.size(), T.get()), *T);
}

using Names = std::vector<std::string>;

std::string name_of(uint32_t len, uint32_t salt) {
  std::string s;
  for (uint32_t b = 0; b < len; ++b) {
    char c = (char)(0x20 + (salt * 11 + b * 5) % 0x5f);
    if (c == '"' || c == '\\') c = '_';
    s.push_back(c);
  }
  return s;
}

void run_select(const std::string& name, const Names& names, bool null_names = false) {
  std::string blob;
  jg_select x{};
  x.n = (uint32_t)names.size();
  for (size_t k = 0; k < names.size(); ++k) {
    if (k < JG_MAX_SELECT) x.name_len[k] = (uint32_t)names[k].size();
    blob += names[k];
  }
  std::unique_ptr<uint8_t[]> keep(new uint8_t[blob.size() + 1]);
  std::memcpy(keep.get(), blob.data(), blob.size());
  x.names = null_names ? nullptr : keep.get();
  auto S = poisoned<Select>();
  show("resolve_select", name, resolve_select(x, S.get()), *S);
}

void run_paths(const std::string& name, const std::vector<Names>& paths, bool null_names = false) {
  std::string blob;
  jg_paths x{};
  x.n = (uint32_t)paths.size();
  for (size_t k = 0; k < paths.size() && k < JG_MAX_PATHS; ++k) {
    x.ncomp[k] = (uint32_t)paths[k].size();
    for (size_t d = 0; d < paths[k].size() && d < JG_PATH_MAX_COMP; ++d) {
      x.comp_len[k][d] = (uint32_t)paths[k][d].size();
      blob += paths[k][d];
    }
  }
  std::unique_ptr<uint8_t[]> keep(new uint8_t[blob.size() + 1]);
  std::memcpy(keep.get(), blob.data(), blob.size());
  x.names = null_names ? nullptr : keep.get();
  auto P = poisoned<Paths>();
  show("resolve_paths", name, resolve_paths(x, P.get()), *P);
}

}  // namespace

int main() {
  const int64_t kMax = std::numeric_limits<int64_t>::max();
  const std::vector<uint32_t> sixteen = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

  // ---- one Expected: resolve(), and the same as a table of one
  run_expect("all_empty", make(0, 0, 0, {}));
  run_expect("empty_iss", make(0, 5, 6, {7, 8}));
  run_expect("empty_sub", make(4, 0, 6, {7, 8}));
  run_expect("empty_jti", make(4, 5, 0, {7, 8}));
  run_expect("empty_aud_first", make(4, 5, 6, {0, 8, 9}));
  run_expect("empty_aud_middle", make(4, 5, 6, {7, 0, 9}));
  run_expect("empty_aud_last", make(4, 5, 6, {7, 8, 0}));
  run_expect("only_auds", make(0, 0, 0, {3, 0, 0, 2}));
  run_expect("sixteen_empty_auds", make(0, 0, 0, std::vector<uint32_t>(16, 0u)));
  run_expect("sixteen_auds", make(20, 30, 36, sixteen, 1700000000, 123456789, 60 * kNsPerSec, 300, 120));
  run_expect("max_bytes_one_string", make(JG_EXPECT_MAX_BYTES, 0, 0, {}));
  run_expect("max_bytes_last_aud", make(0, 0, 0, {1, JG_EXPECT_MAX_BYTES - 1}));
  run_expect("max_bytes_spread", make(1000, 1000, 1000, {500, 500, 96}));
  run_expect("negative_now_largest_skew", make(3, 0, 0, {2}, -5, 999999999u, kMax, -7, 9));
  run_expect("negative_now_before_year_1", make(0, 0, 0, {}, -62135596801LL, 1, 1500000000LL));
  run_expect("negative_skew", make(0, 2, 0, {}, 1700000000, 5, -2500000000LL));
  run_expect("nsec_carry", make(0, 0, 0, {}, 1700000000, 999999999u, 1, 1, 1));
  // refused
  run_expect("over_max_bytes", make(JG_EXPECT_MAX_BYTES, 1, 0, {}));
  run_expect("over_max_bytes_in_auds", make(0, 0, 0, {4000, 97}));
  run_expect("nsec_1e9", make(1, 1, 1, {}, 1700000000, 1000000000u));
  run_expect("null_strs", make(1, 0, 0, {}), true);
  {
    Ex e = make(1, 1, 1, sixteen);
    e.x.naud = 17;
    run_expect("seventeen_auds", e);
  }

  // ---- tables: resolve_profiles()
  {
    std::vector<Ex> es;
    for (uint32_t p = 0; p < JG_MAX_PROFILES; ++p)
      es.push_back(make(p % 5, (p + 1) % 3, p % 2, {p % 7, 3}, 1700000000 + p, p, (int64_t)p * kNsPerSec, p, 2 * p));
    run_profiles("sixty_four", es);
    es.push_back(make(1, 1, 1, {}));
    run_profiles("sixty_five", es);                                     // refused
  }
  {
    std::vector<Ex> es(JG_MAX_PROFILES, make(40, 24, 0, {32, 0, 32}));  // 64 x 128 bytes
    run_profiles("pool_full_sixty_four", es);
    es[63] = make(40, 24, 1, {32, 0, 32});
    run_profiles("pool_over_by_one", es);                               // refused
  }
  run_profiles("pool_full_two", {make(JG_EXPECT_MAX_BYTES, 0, 0, {}), make(0, 96, 0, {4000})});
  run_profiles("pool_full_then_empty", {make(JG_EXPECT_MAX_BYTES, 0, 0, {}), make(0, 96, 0, {4000}), make(0, 0, 0, {})});
  run_profiles("pool_full_then_one_byte", {make(JG_EXPECT_MAX_BYTES, 0, 0, {}), make(0, 96, 0, {4000}), make(0, 0, 1, {})});
  run_profiles("empty_between", {make(3, 0, 2, {0, 4}), make(0, 0, 0, {}), make(0, 5, 0, {1, 0})});
  run_profiles("negative_now_largest_skew_second", {make(2, 2, 2, sixteen), make(3, 0, 0, {2}, -5, 999999999u, kMax, -7, 9)});
  run_profiles("none", {});                                             // refused
  run_profiles("second_over_max_bytes", {make(1, 1, 1, {}), make(JG_EXPECT_MAX_BYTES, 1, 0, {})});
  run_profiles("second_nsec_1e9", {make(1, 1, 1, {}), make(1, 1, 1, {}, 0, 1000000000u)});
  run_profiles("null_strs", {make(1, 1, 1, {}), make(0, 0, 0, {2})}, true);
  {
    auto T = poisoned<Profiles>();
    show("resolve_profiles", "null_expects", resolve_profiles(nullptr, 1, T.get()), *T);
  }

  // ---- names: resolve_select()
  run_select("none", {});
  run_select("one", {"scope"});
  run_select("eight_of_64", {name_of(64, 1), name_of(64, 2), name_of(64, 3), name_of(64, 4), name_of(64, 5), name_of(64, 6),
                             name_of(64, 7), name_of(64, 8)});
  run_select("mixed_lengths", {"a", name_of(64, 9), "ab", "b", name_of(63, 9), "realm_access", " ", "~"});
  run_select("prefixes_and_case", {"role", "roles", "Role", "rol"});
  run_select("nine", {"a", "b", "c", "d", "e", "f", "g", "h", "i"});    // refused from here on
  run_select("empty_name", {"a", ""});
  run_select("65_bytes", {name_of(65, 1)});
  run_select("byte_1f", {std::string("a\x1f" "b")});
  run_select("byte_7f", {std::string("a\x7f")});
  run_select("byte_80", {std::string("\x80" "a")});
  run_select("byte_00", {std::string("a\0b", 3)});
  run_select("quote", {"a\"b"});
  run_select("backslash", {"a", "b\\"});
  run_select("equal_names", {"a", "b", "a"});
  run_select("equal_names_of_64", {name_of(64, 1), name_of(64, 2), name_of(64, 1)});
  run_select("null_names", {"a"}, true);

  // ---- paths: resolve_paths()
  run_paths("none", {});
  run_paths("one", {{"realm_access", "roles"}});
  {
    std::vector<Names> full;
    for (uint32_t k = 0; k < JG_MAX_PATHS; ++k)
      full.push_back({name_of(64, 4 * k), name_of(64, 4 * k + 1), name_of(64, 4 * k + 2), name_of(64, 4 * k + 3)});
    run_paths("eight_of_4_of_64", full);
  }
  run_paths("eight_of_4", {{"a", "b", "c", "d"}, {"a", "b", "c", "e"}, {"a", "b", "x", "d"}, {"a", "y", "c", "d"},
                           {"z", "b", "c", "d"}, {"a", "b", "c", "dd"}, {"aa", "b", "c", "d"}, {"a", "bb", "c", "d"}});
  run_paths("prefixes", {{"a"}, {"a", "b"}, {"a", "b", "c"}, {"a", "b", "c", "d"}});
  run_paths("mixed_counts", {{"a", "b"}, {"ab"}, {"b", "a"}, {"a", "B"}, {" ~", "a.b", "a/b"}});
  run_paths("nine", {{"a"}, {"b"}, {"c"}, {"d"}, {"e"}, {"f"}, {"g"}, {"h"}, {"i"}});   // refused from here on
  run_paths("no_component", {{"a"}, {}});
  run_paths("five_components", {{"a", "b", "c", "d", "e"}});
  run_paths("empty_component", {{"a", ""}});
  run_paths("empty_first_component", {{"", "a"}});
  run_paths("65_bytes", {{"a", name_of(65, 1)}});
  run_paths("byte_1f", {{"a", std::string("a\x1f" "b")}});
  run_paths("byte_7f", {{std::string("a\x7f" "b")}});
  run_paths("byte_80", {{"a", "b", std::string("a\x80" "b")}});
  run_paths("byte_00", {{"a", std::string("a\0b", 3)}});
  run_paths("quote", {{"a", "a\"b"}});
  run_paths("backslash", {{"a\\b", "c"}});
  run_paths("equal_paths", {{"a", "b"}, {"c"}, {"a", "b"}});
  run_paths("equal_paths_of_4", {{"a", "b", "c", "d"}, {"x"}, {"a", "b", "c", "d"}});
  run_paths("null_names", {{"a"}}, true);
  return 0;
}
