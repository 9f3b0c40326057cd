// match_set.cpp -- the MatchArgs entries with InSet / AnyElementIn and ClaimSet
// without a GPU, linked with match_set_stub.cpp; or, run as `match_set nolib` and
// linked with tests/host_match_hash/match_hash_stub.cpp alone, against a library
// that has neither jg_set_* nor jg_claims_match_set.
//
// The tokens are made here (RS256 headers; the stand-in accepts every signature)
// with the mask Go code on the claims map owes under reqs() below, written out by
// hand beside each.  Checked: bits, ok and stats of MatchBatchArgs; ok / err
// against CheckBatch; one jg_claims_match_set call per batch and none of the older
// entries; the Verdicts and *Each forms; a host-only set and five sets give the
// same bits from the host path without a call of the ABI; four sets are scanned;
// Replace under the failure policy on both paths; Close; the 17th set; the seed;
// what throws.  Prints FAIL lines and exits 1 on a mismatch.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/host/cap_jwt.hpp"
#include "../../include/jg.h"

using namespace capjwt;

extern "C" int match_args_stub_calls;
extern "C" int match_hash_stub_calls;
extern "C" __attribute__((weak)) int match_set_stub_calls;
extern "C" __attribute__((weak)) int match_set_stub_refused;
extern "C" __attribute__((weak)) int match_set_stub_nsets;
extern "C" __attribute__((weak)) int set_stub_loads;
extern "C" __attribute__((weak)) int set_stub_frees;
extern "C" __attribute__((weak)) int set_stub_fail;
extern "C" __attribute__((weak)) uint32_t set_stub_last_seed;

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
static std::string token(const std::string& payload) {
  return b64("{\"alg\":\"RS256\"}") + "." + b64(payload) + "." + std::string(342, 'A');
}

using R = Require;
static Require req(ClaimPath path, R::Op op, const ClaimSet& set = ClaimSet(), uint32_t column = 0) {
  Require r;
  r.path = std::move(path);
  r.op = op;
  r.column = column;
  r.set = set;
  return r;
}
// bit 0 sid in `revoked`, 1 groups has an element in `groups`, 2 groups in `groups`, 3 nonce = the token's own, 4 sid is a string
static std::vector<Require> reqs(const ClaimSet& revoked, const ClaimSet& groups) {
  return {req({"sid"}, R::InSet, revoked), req({"groups"}, R::AnyElementIn, groups), req({"groups"}, R::InSet, groups),
          req({"nonce"}, R::EqualsArg), req({"sid"}, R::IsString)};
}

struct Case {
  std::string payload, nonce;
  bool ok, host;
  uint32_t bits;
};

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

int main(int argc, char** argv) {
  const bool nolib = argc == 2 && std::string(argv[1]) == "nolib";
  const std::string exp = ",\"nonce\":\"n-1\",\"exp\":1611699944}", old = ",\"nonce\":\"n-1\",\"exp\":1611692144}";
  const std::string longm(255, 'L');
  const std::vector<Case> cases = {
      {"{\"sid\":\"jti-1\",\"groups\":[\"admin\"]" + exp, "n-1", true, false, 0b11011},
      {"{\"sid\":\"jti-2\",\"groups\":\"admin\"" + exp, "n-1", true, false, 0b11100},
      {"{\"sid\":\"\",\"groups\":[]" + exp, "n-1", true, false, 0b11001},
      {"{\"sid\":\"jti\\u002d1\",\"groups\":[\"x\",\"ops\"]" + exp, "n-1", true, true, 0b11011},     // an escape: the host path
      {"{\"sid\":7" + exp, "n-1", true, false, 0b01000},
      {"{\"sid\":\"jti-1\",\"groups\":[\"admin\"]" + old, "n-1", false, false, 0},                    // expired: scanned, rejected
      {"", "n-1", false, false, 0},                                                                   // no JWT at all
      {"{\"sid\":\"abc\",\"groups\":[[\"admin\"],{\"admin\":\"admin\"},7]" + exp, "n-2", true, false, 0b10001},
      {"{\"sid\":\"\xc3\xa9\",\"groups\":[\"x\",7,\"admin\"]" + exp, "n-1", true, false, 0b11010},
      {"{\"sid\":\"" + longm + "\",\"groups\":[\"admin \"]" + exp, "n-1", true, false, 0b11001},
      {"{\"sid\":\"" + longm + "L\",\"sid\":\"jti-1\",\"sid\":\"nope\"" + exp, "n-1", true, false, 0b11000},   // the last member wins
  };
  const size_t n = cases.size();
  std::vector<std::string> store;
  for (const Case& c : cases) store.push_back(c.payload.empty() ? std::string("not-a-jwt") : token(c.payload));
  std::vector<std::string_view> toks(store.begin(), store.end());
  std::vector<std::vector<std::string_view>> strs(1);
  for (const Case& c : cases) strs[0].push_back(c.nonce);
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

  const std::vector<std::string> revoked_m = {"jti-1", "", "abc", longm, "jti-1", "revoked-9"}, groups_m = {"admin", "ops"};
  ClaimSet revoked = v->NewClaimSet(revoked_m, 7u), groups = v->NewClaimSet(groups_m);
  check(revoked.size() == 5 && groups.size() == 2, "duplicates fold", std::to_string(revoked.size()));
  const std::vector<Require> rq = reqs(revoked, groups);

  if (nolib) {
    // the library has no jg_set_* and no jg_claims_match_set: the handles exist, the tokens the scan would carry get
    // its unavailable error, and a call without a set requirement works as ever
    check(&match_set_stub_calls == nullptr, "the stand-in without the set entries is linked");
    check(!revoked.info().host_only && revoked.info().nslots == 0, "a handle without the ABI");
    const auto rs = v->MatchBatchArgs(toks, ex, rq, strs, nums);
    size_t unavailable = 0;
    for (size_t i = 0; i < n; ++i) {
      const bool un = rs[i].err.find("capjwt: claims scan unavailable: ") == 0 && rs[i].err.find("jg_claims_match_set") != std::string::npos;
      unavailable += un;
      if (un) check(!rs[i].ok && rs[i].bits == 0 && !cases[i].payload.empty(), "unavailable: token " + std::to_string(i));
    }
    // every token the scan carried, the one it would have left to the host included: as after any failed scan
    check(unavailable == n - 1, "the scan is reported unavailable per token", std::to_string(unavailable));
    const auto r2 = v->MatchBatchArgs(toks, ex, {rq[3], rq[4]}, strs, nums);
    for (size_t i = 0; i < n; ++i)
      check(r2[i].ok == cases[i].ok && r2[i].bits == (cases[i].ok ? (cases[i].bits >> 3) & 3u : 0u), "without a set requirement: token " + std::to_string(i), r2[i].err);
    if (fails) return 1;
    std::printf("match set nolib: ok\n");
    return 0;
  }

  check(revoked.info().seed == 7u && revoked.info().n == 5 && !revoked.info().host_only && revoked.info().nslots == 16 &&
            revoked.info().generation == 1,
        "info of a resident set", std::to_string(revoked.info().seed) + " " + std::to_string(revoked.info().nslots));
  {
    ClaimSet a = v->NewClaimSet({"x"}), b = v->NewClaimSet({"x"});
    ClaimSet c = v->NewClaimSet({"x"}), d = v->NewClaimSet({"x"});
    const uint32_t s[4] = {a.info().seed, b.info().seed, c.info().seed, d.info().seed};
    check(!(s[0] == s[1] && s[1] == s[2] && s[2] == s[3]), "the seed is random per load");
  }

  size_t want_host = 0, want_scanned = 0;
  for (const Case& c : cases) {
    want_host += !c.payload.empty() && c.host;
    want_scanned += !c.payload.empty() && !c.host;
  }
  CheckStats st;
  const int s0 = match_set_stub_calls, h0 = match_hash_stub_calls, a0 = match_args_stub_calls;
  const auto rs = v->MatchBatchArgs(toks, ex, rq, strs, nums, &st);
  const auto cs = v->CheckBatch(toks, ex);
  check(match_set_stub_calls == s0 + 1 && match_hash_stub_calls == h0 && match_args_stub_calls == a0,
        "one jg_claims_match_set call and none of the older entries", std::to_string(match_set_stub_calls - s0));
  check(match_set_stub_refused == 0 && match_set_stub_nsets == 2, "the ABI took the host's call with two sets");
  check(st.host == want_host && st.scanned == want_scanned, "stats", std::to_string(st.scanned) + " scanned, " + std::to_string(st.host) + " host");
  for (size_t i = 0; i < n; ++i) {
    const std::string at = "token " + std::to_string(i);
    check(rs[i].ok == cs[i].ok && rs[i].err == cs[i].err, at + " differs from CheckBatch", rs[i].err + " / " + cs[i].err);
    check(rs[i].ok == cases[i].ok, at + " ok", rs[i].err);
    check(rs[i].bits == cases[i].bits, at + " bits", std::to_string(rs[i].bits) + " / " + std::to_string(cases[i].bits));
  }
  // the Verdicts and the *Each forms hold the same rows
  {
    std::vector<uint8_t> ok(n, 0xee);
    std::vector<uint32_t> bits(n, 0xeeeeeeeeu);
    v->MatchVerdictsArgs(toks, ex, rq, strs, nums, ok.data(), bits.data());
    for (size_t i = 0; i < n; ++i) check(ok[i] == (rs[i].ok ? 1 : 0) && bits[i] == rs[i].bits, "MatchVerdictsArgs token " + std::to_string(i));
    Expected late = ex;
    late.now_unix_ns = (1611699344LL + 7200) * 1000000000LL;
    const std::vector<Expected> es = {ex, late};
    std::vector<uint32_t> which(n);
    for (size_t i = 0; i < n; ++i) which[i] = (uint32_t)(i % 2);
    const auto each = v->MatchBatchArgsEach(toks, es, which, rq, strs, nums);
    v->MatchVerdictsArgsEach(toks, es, which, rq, strs, nums, ok.data(), bits.data());
    const auto other = v->MatchBatchArgs(toks, late, rq, strs, nums);
    size_t rejected = 0;
    for (size_t i = 0; i < n; ++i) {
      const MatchResult& alone = i % 2 ? other[i] : rs[i];
      check(each[i].ok == alone.ok && each[i].err == alone.err && each[i].bits == alone.bits, "MatchBatchArgsEach token " + std::to_string(i));
      check(ok[i] == (alone.ok ? 1 : 0) && bits[i] == alone.bits, "MatchVerdictsArgsEach token " + std::to_string(i));
      rejected += i % 2 && rs[i].ok && !alone.ok;
    }
    check(rejected >= 2, "the later clock rejects tokens", std::to_string(rejected));
  }
  // a host-only set: a member the device refuses.  No call of the ABI, every token from the host path, and the one
  // payload whose sid is that member now holds bit 0
  for (const std::string& extra : {std::string("\xc3\xa9"), std::string(256, 'x') , std::string("q\"q"), std::string("a\x1f")}) {
    std::vector<std::string> m = revoked_m;
    m.push_back(extra);
    ClaimSet ho = v->NewClaimSet(m);
    check(ho.info().host_only && ho.info().n == 6 && ho.info().nslots == 0, "a host-only set says so");
    CheckStats s2;
    const int c1 = match_set_stub_calls;
    const auto r2 = v->MatchBatchArgs(toks, ex, reqs(ho, groups), strs, nums, &s2);
    check(match_set_stub_calls == c1 && s2.scanned == 0 && s2.host == want_host + want_scanned, "a host-only set reaches the ABI");
    for (size_t i = 0; i < n; ++i)
      check(r2[i].ok == rs[i].ok && r2[i].bits == (rs[i].bits | (i == 8 && extra == "\xc3\xa9" ? 1u : 0u)), "host-only set: token " + std::to_string(i),
            std::to_string(r2[i].bits));
  }
  // four sets are scanned; five are not, and give the same bits
  {
    std::vector<ClaimSet> five;
    for (int k = 0; k < 5; ++k) five.push_back(v->NewClaimSet(revoked_m));
    std::vector<Require> r4, r5;
    for (int k = 0; k < 5; ++k) {
      if (k < 4) r4.push_back(req({"sid"}, R::InSet, five[k]));
      r5.push_back(req({"sid"}, R::InSet, five[k]));
    }
    r4.push_back(req({"sid"}, R::InSet, five[0]));                                // the same handle again: no fifth set
    CheckStats s4, s5;
    const int c1 = match_set_stub_calls;
    const auto q4 = v->MatchBatchArgs(toks, ex, r4, strs, nums, &s4);
    check(match_set_stub_calls == c1 + 1 && match_set_stub_nsets == 4 && s4.scanned == want_scanned, "four sets are scanned");
    const auto q5 = v->MatchBatchArgs(toks, ex, r5, strs, nums, &s5);
    check(match_set_stub_calls == c1 + 1 && s5.scanned == 0 && s5.host == want_host + want_scanned, "five sets reach the ABI");
    for (size_t i = 0; i < n; ++i) {
      const uint32_t b = rs[i].bits & 1u;
      check(q4[i].bits == (b ? 31u : 0u) && q5[i].bits == (b ? 31u : 0u) && q4[i].ok == rs[i].ok && q5[i].ok == rs[i].ok,
            "four / five sets: token " + std::to_string(i), std::to_string(q4[i].bits) + " / " + std::to_string(q5[i].bits));
    }
    // the 17th live set: revoked, groups and these five are live; nine more fit
    std::vector<ClaimSet> more;
    for (int k = 0; k < 9; ++k) more.push_back(v->NewClaimSet({"m"}));
    check(throws<std::runtime_error>([&] { (void)v->NewClaimSet({"m"}); }), "the 17th set throws");
    more.pop_back();                                                              // the last copy dies: its id is free again
    ClaimSet again = v->NewClaimSet({"m"});
    check(again.size() == 1, "an id freed by the handle is taken again");
    more[0].Close();
    ClaimSet third = v->NewClaimSet({"m"});
    check(throws<std::runtime_error>([&] { (void)v->NewClaimSet({"m"}); }), "sixteen are live again");
  }
  // Replace: the whole set anew under the same id; a failure leaves the old one in force on both paths
  {
    const int l0 = set_stub_loads;
    revoked.Replace({"jti-2", "jti-2"}, 9u);
    check(set_stub_loads == l0 + 1 && set_stub_last_seed == 9u && revoked.size() == 1 && revoked.info().generation > 1, "Replace loads");
    auto r2 = v->MatchBatchArgs(toks, ex, rq, strs, nums);
    for (size_t i = 0; i < n; ++i)
      check(r2[i].bits == ((rs[i].bits & ~1u) | (i == 1 ? 1u : 0u)), "after Replace: token " + std::to_string(i), std::to_string(r2[i].bits));
    revoked.Replace(revoked_m);
    set_stub_fail = 1;
    check(throws<std::runtime_error>([&] { revoked.Replace({"jti-2"}); }), "a failed load throws");
    check(throws<std::runtime_error>([&] { (void)v->NewClaimSet({"m"}); }), "a failed first load throws");
    set_stub_fail = 0;
    check(throws<std::invalid_argument>([&] { revoked.Replace({"ok", std::string("nul\0x", 5)}); }), "a NUL in a member throws");
    check(throws<std::invalid_argument>([&] { (void)v->NewClaimSet({std::string(1, '\0')}); }), "a NUL in a first member throws");
    check(revoked.size() == 5, "the old members stay");
    r2 = v->MatchBatchArgs(toks, ex, rq, strs, nums);
    for (size_t i = 0; i < n; ++i) check(r2[i].bits == rs[i].bits && r2[i].ok == rs[i].ok, "after the failures: token " + std::to_string(i));
    ClaimSet fits = v->NewClaimSet({"m"});                                        // the failed first loads kept no id
    // to a host-only set and back
    std::vector<std::string> m = revoked_m;
    m.push_back("\xc3\xa9");
    revoked.Replace(m);
    check(revoked.info().host_only, "Replace to a host-only set");
    const int c1 = match_set_stub_calls;
    r2 = v->MatchBatchArgs(toks, ex, rq, strs, nums);
    check(match_set_stub_calls == c1 && r2[8].bits == (rs[8].bits | 1u) && r2[0].bits == rs[0].bits, "a replaced, host-only set");
    revoked.Replace(revoked_m);
    check(!revoked.info().host_only && revoked.info().n == 5, "... and back");
  }
  // Close: the id is freed now, and a call that names the set throws
  {
    const int f0 = set_stub_frees;
    ClaimSet copy = groups;
    groups.Close();
    check(set_stub_frees == f0 + 1, "Close frees the id");
    check(throws<std::invalid_argument>([&] { (void)v->MatchBatchArgs(toks, ex, rq, strs, nums); }), "a closed set throws");
    check(throws<std::invalid_argument>([&] { copy.Replace({"x"}); }), "Replace on a closed set throws");
    copy.Close();
    check(set_stub_frees == f0 + 1, "Close twice frees once");
  }
  // what no path takes
  {
    ClaimSet live = v->NewClaimSet(groups_m);
    check(throws<std::invalid_argument>([&] { (void)v->MatchBatchArgs(toks, ex, {req({"sid"}, R::InSet)}, strs, nums); }), "InSet without a set throws");
    check(throws<std::invalid_argument>([&] { (void)v->MatchBatch(toks, ex, {req({"sid"}, R::InSet, live)}); }), "MatchBatch takes InSet");
    check(throws<std::invalid_argument>([&] { (void)v->MatchBatchArgs(toks, ex, {req({"a"}, (R::Op)14, live)}, strs, nums); }), "an unknown op throws");
    check(throws<std::invalid_argument>([&] { (void)match_requires(json::Value{}, {req({"a"}, R::InSet, live)}, {}, {}); }),
          "match_requires without hash columns takes InSet");
    auto ks2 = NewStaticKeySet({rsa}, &err);
    auto v2 = NewValidator(ks2.get(), &err);
    check(throws<std::invalid_argument>([&] { (void)v2->MatchBatchArgs(toks, ex, {req({"sid"}, R::InSet, live)}, strs, nums); }),
          "a set of another key set throws");
    check(v->MatchBatchArgs({}, ex, {req({"sid"}, R::InSet, live)}, {{}}, {}).empty(), "an empty batch");
    // match_requires on a claims map, as the host path runs it
    json::Value doc;
    std::string perr;
    check(json::parse("{\"sid\":\"ops\",\"groups\":[\"x\",[\"ops\"],\"ops\"],\"n\":1}", &doc, &perr), "parse", perr);
    check(match_requires(doc, {req({"sid"}, R::InSet, live), req({"groups"}, R::AnyElementIn, live), req({"groups"}, R::InSet, live),
                               req({"sid"}, R::AnyElementIn, live), req({"n"}, R::InSet, live), req({"gone"}, R::InSet, live)},
                         {}, {}, {}) == 0b000011, "match_requires with sets");
  }
  if (fails) return 1;
  std::printf("match set: ok\n");
  return 0;
}
