// set_add.cpp -- ClaimSet::Add without a GPU, linked with set_add_stub.cpp; the
// same program linked with the stand-in built -DNO_SET_ADD runs against a library
// without jg_set_add, where an Add reloads the union whole with the same results.
//
// The tokens are made here (RS256 headers; the stand-in accepts every signature);
// the one requirement is InSet("sid", set), so bit 0 of a token says whether its
// sid is a member.  Token 2 spells its sid with an escape and takes the host path;
// the others are scanned.  Checked: Add is visible on both paths; the count it
// returns with repeats and resident members; only new members reach the ABI;
// nothing new makes no call; a failed add and a NUL leave both paths on the old
// members; after a lost context recover() loads the added members again; a few
// hundred single adds (the host copy's overlay folds); the transition to
// host-only and Add on a host-only set; Add after Replace; Add after Close.
// Prints FAIL lines and exits 1 on a mismatch.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/host/cap_jwt.hpp"
#include "../../include/jg.h"

using namespace capjwt;

extern "C" int match_set_stub_calls;
extern "C" int set_stub_loads;
extern "C" int set_stub_fail;
extern "C" int set_add_stub_calls;
extern "C" int set_add_stub_given;
extern "C" int set_add_stub_fail;
extern "C" int set_add_stub_lose;
extern "C" int set_add_stub_present;

static int fails = 0;
static void check(bool ok, const std::string& what, const std::string& got = "") {
  if (!ok) {
    std::printf("FAIL %s: %s\n", what.c_str(), got.c_str());
    ++fails;
  }
}

static std::string b64(const std::string& in) {
  static const char* A = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_";
  std::string o;
  size_t i = 0;
  for (; i + 2 < in.size(); i += 3) {
    const uint32_t v = (uint8_t)in[i] << 16 | (uint8_t)in[i + 1] << 8 | (uint8_t)in[i + 2];
    o += A[v >> 18]; o += A[(v >> 12) & 63]; o += A[(v >> 6) & 63]; o += A[v & 63];
  }
  if (in.size() - i == 1) {
    const uint32_t v = (uint8_t)in[i] << 16;
    o += A[v >> 18]; o += A[(v >> 12) & 63];
  } else if (in.size() - i == 2) {
    const uint32_t v = (uint8_t)in[i] << 16 | (uint8_t)in[i + 1] << 8;
    o += A[v >> 18]; o += A[(v >> 12) & 63]; o += A[(v >> 6) & 63];
  }
  return o;
}
static std::string token(const std::string& sid_json) {
  return b64("{\"alg\":\"RS256\"}") + "." + b64("{\"sid\":\"" + sid_json + "\",\"exp\":1611699944}") + "." + std::string(342, 'A');
}

template <class E, class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const E&) {
    return true;
  } catch (...) {
  }
  return false;
}

int main() {
  const bool has_add = set_add_stub_present != 0;
  // sids: 0 jti-1, 1 jti-2, 2 jti-3 (escaped: the host path), 3 new-1, 4 e-acute, 5 bulk-150, 6 bulk-299 (escaped)
  const std::vector<std::string> sids = {"jti-1", "jti-2", "jti\\u002d3", "new-1", "\xc3\xa9", "bulk-150", "bulk\\u002d299"};
  std::vector<std::string> store;
  for (const std::string& s : sids) store.push_back(token(s));
  const std::vector<std::string_view> toks(store.begin(), store.end());
  const size_t n = toks.size();
  const std::vector<std::vector<std::string_view>> strs;
  const std::vector<const int64_t*> nums;

  PublicKey rsa;
  rsa.kind = PublicKey::RSA;
  rsa.n = std::string(256, '\xc5');
  rsa.e = 65537;
  std::string err;
  auto ks = NewStaticKeySet({rsa}, &err);
  check(ks != nullptr, "static key set", err);
  if (!ks) return 1;
  auto v = NewValidator(ks.get(), &err);
  Expected ex;
  ex.SigningAlgorithms = {"RS256"};
  ex.has_now = true;
  ex.now_unix_ns = 1611699344LL * 1000000000LL;
  ex.NotBeforeLeeway = 3600 * 1000000000LL;

  ClaimSet s = v->NewClaimSet({"jti-1"}, 7u);
  ClaimSet other = v->NewClaimSet({"kept"});                                      // a second live set, untouched throughout
  Require rq;
  rq.path = {"sid"};
  rq.op = Require::InSet;
  rq.set = s;
  // the bits of the seven tokens as a string, and how many were scanned / answered by the host path
  CheckStats st;
  const auto bits = [&]() {
    const auto rs = v->MatchBatchArgs(toks, ex, {rq}, strs, nums, &st);
    std::string o;
    for (size_t i = 0; i < n; ++i) o += !rs[i].ok ? 'x' : rs[i].bits ? '1' : '0';
    return o;
  };
  // the device calls an Add of `given` new members must have made since (a0, l0)
  const auto went_to_device = [&](int a0, int l0, int given) {
    return has_add ? set_add_stub_calls == a0 + 1 && set_add_stub_given == given && set_stub_loads == l0
                   : set_stub_loads == l0 + 1;
  };
  check(bits() == "1000000" && st.scanned == 5 && st.host == 2, "before any add", bits());

  // Add is visible on both paths; repeats and resident members do not count and do not reach the ABI
  int a0 = set_add_stub_calls, l0 = set_stub_loads, g0 = set_add_stub_given;
  uint64_t gen = s.info().generation;
  check(s.Add({"jti-2", "jti-3", "jti-2", "jti-1"}) == 2, "Add returns the new members");
  check(went_to_device(a0, l0, g0 + 2), "two members reach the device", std::to_string(set_add_stub_given - g0));
  check(bits() == "1110000" && st.scanned == 5 && st.host == 2, "after Add: the scan path (1) and the host path (2)", bits());
  check(s.size() == 3 && s.info().n == 3 && !s.info().host_only && s.info().generation > gen, "info after Add");
  if (has_add) check(s.info().seed == 7u, "the seed stays");
  // nothing new: no call of the ABI
  a0 = set_add_stub_calls, l0 = set_stub_loads, gen = s.info().generation;
  check(s.Add({"jti-1", "jti-2"}) == 0 && s.Add({}) == 0, "nothing new returns 0");
  check(set_add_stub_calls == a0 && set_stub_loads == l0 && s.info().generation == gen, "nothing new makes no device call");
  // a failed add, and a NUL: the old members stay in force on both paths
  (has_add ? set_add_stub_fail : set_stub_fail) = 1;
  check(throws<std::runtime_error>([&] { (void)s.Add({"new-1"}); }), "a failed add throws runtime_error");
  (has_add ? set_add_stub_fail : set_stub_fail) = 0;
  check(throws<std::invalid_argument>([&] { (void)s.Add({"new-1", std::string("nul\0x", 5)}); }), "a NUL in a member throws");
  check(s.size() == 3 && s.info().generation == gen && bits() == "1110000", "after the failures", bits());
  // the context is lost: the failed call's tokens are unavailable, recover() loads the sets again with what was added
  l0 = set_stub_loads;
  set_add_stub_lose = 1;
  const std::string lost = bits();
  check(lost == "xxxxxxx", "the call that loses the context", lost);
  check(set_stub_loads == l0 + 2, "recover loads both live sets again", std::to_string(set_stub_loads - l0));
  check(bits() == "1110000" && st.scanned == 5 && s.info().n == 3, "after recover the added members are there", bits());
  check(s.Add({"new-1"}) == 1 && bits() == "1111000", "an add after recover", bits());
  // single adds, one at a time: the host copy's overlay folds into its base on the way
  a0 = set_add_stub_calls;
  size_t cnt = 0;
  for (int k = 0; k < 300; ++k) cnt += s.Add({"bulk-" + std::to_string(k), "jti-1"});
  check(cnt == 300 && s.size() == 304 && s.info().n == 304, "300 single adds", std::to_string(s.size()));
  if (has_add) check(set_add_stub_calls == a0 + 300, "one jg_set_add each");
  check(bits() == "1111011" && st.host == 2, "members added one by one, on both paths", bits());
  l0 = set_stub_loads;
  set_add_stub_lose = 1;
  (void)bits();
  check(set_stub_loads == l0 + 2 && bits() == "1111011", "recover after many adds", bits());
  // a member the device refuses: host-only from here on, the id kept with nothing in it
  int c0;
  check(s.Add({"ok-1", "\xc3\xa9"}) == 2 && s.info().host_only && s.info().nslots == 0 && s.size() == 306, "Add turns the set host-only");
  c0 = match_set_stub_calls;
  check(bits() == "1111111" && match_set_stub_calls == c0 && st.scanned == 0 && st.host == 7, "a host-only set is answered by the host path", bits());
  a0 = set_add_stub_calls, l0 = set_stub_loads;
  check(s.Add({"ho-1", "ho-1", "jti-1"}) == 1 && s.size() == 307 && s.info().host_only, "Add on a host-only set");
  check(set_add_stub_calls == a0 && set_stub_loads == l0, "... touches the host copy alone");
  // a failed transition leaves the set resident with its members
  {
    ClaimSet t = v->NewClaimSet({"a"});
    set_stub_fail = 1;
    check(throws<std::runtime_error>([&] { (void)t.Add({"b", "\x01"}); }), "a failed transition throws");
    set_stub_fail = 0;
    check(t.size() == 1 && !t.info().host_only && t.info().n == 1, "... and leaves the set");
  }
  // Replace brings it back; Add goes to the device again
  s.Replace({"jti-1"});
  a0 = set_add_stub_calls, l0 = set_stub_loads, g0 = set_add_stub_given;
  check(s.Add({"jti-2"}) == 1 && went_to_device(a0, l0, g0 + 1) && !s.info().host_only, "Add after Replace");
  check(bits() == "1100000" && st.scanned == 5, "after Replace and Add", bits());
  check(other.size() == 1 && other.info().n == 1, "the other set is untouched");
  ClaimSet copy = s;
  s.Close();
  check(throws<std::invalid_argument>([&] { (void)copy.Add({"late"}); }), "Add after Close throws");
  check(throws<std::invalid_argument>([&] { (void)ClaimSet().Add({"x"}); }), "Add on an empty handle throws");
  if (fails) return 1;
  std::printf("set add%s: ok\n", has_add ? "" : " without jg_set_add");
  return 0;
}
