// match_hash.cpp -- the MatchArgs entries with hash columns (HashOfArg,
// IsString) without a GPU, linked with match_hash_stub.cpp.
//
//   match_hash CASES
//
// CASES is written by tests/test_host_match_hash.py, one token per line:
//   <token> <nonce> <access token in hex, "-" = none> <code in hex, "-" = none> <ok> <host> <bits>
// with the mask the plain-Python evaluation on the oracle's claims map owes under
// kReqs below, whether the token is accepted and whether it takes the host path.
// Checked: bits, ok and the stats of MatchBatchArgs; ok / err against CheckBatch;
// one jg_claims_match_hash call per batch and no jg_claims_match_args call; the
// families the ABI receives; one jg_hash_batch call over just the host-path
// tokens' values; MatchVerdictsArgs and the *Each forms; a list over the caps
// gives the same bits from the host path; a call without hash columns or new ops
// still goes through jg_claims_match_args; a failed jg_hash_batch surfaces as the
// scan's unavailable error; what throws.
// Prints FAIL lines and exits 1 on a mismatch.
#include <cstdio>
#include <fstream>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/host/cap_jwt.hpp"
#include "../../include/jg.h"

using namespace capjwt;

extern "C" int match_args_stub_calls;
extern "C" int match_hash_stub_calls;
extern "C" int match_hash_stub_refused;
extern "C" int match_hash_stub_sources;
extern "C" int hash_stub_calls;
extern "C" int hash_stub_jobs;
extern "C" int hash_stub_fail;

static int fails = 0;
static void check(bool ok, const std::string& what, const std::string& got = "") {
  if (!ok) {
    std::printf("FAIL %s: %s\n", what.c_str(), got.c_str());
    ++fails;
  }
}

static std::string unhex(const std::string& h) {
  std::string o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return o;
}

using R = Require;
static Require req(ClaimPath path, R::Op op, uint32_t column = 0, std::string value = "") {
  Require r;
  r.path = std::move(path);
  r.op = op;
  r.value = std::move(value);
  r.column = column;
  return r;
}
// bit 0 up
static const std::vector<Require> kReqs = {req({"nonce"}, R::EqualsArg, 0), req({"at_hash"}, R::HashOfArg, 0),
                                           req({"at_hash"}, R::IsString),   req({"c_hash"}, R::HashOfArg, 1),
                                           req({"c_hash"}, R::IsString)};

struct Case {
  std::string token, nonce;
  std::optional<std::string> at, code;
  bool ok, host;
  uint32_t bits;
};

template <class F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::vector<Case> cases;
  {
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      std::istringstream ss(line);
      Case c;
      std::string at, code;
      int ok = 0, host = 0;
      ss >> c.token >> c.nonce >> at >> code >> ok >> host >> c.bits;
      if (!ss) {
        std::printf("bad line: %s\n", line.c_str());
        return 2;
      }
      if (c.nonce == "-") c.nonce.clear();
      if (at != "-") c.at = unhex(at == "+" ? "" : at);
      if (code != "-") c.code = unhex(code == "+" ? "" : code);
      c.ok = ok;
      c.host = host;
      cases.push_back(std::move(c));
    }
  }
  check(cases.size() >= 12, "the cases");
  const size_t n = cases.size();
  std::vector<std::string_view> toks;
  std::vector<std::vector<std::string_view>> strs(1);
  std::vector<HashColumn> hashes(2);
  for (const Case& c : cases) {
    toks.push_back(c.token);
    strs[0].push_back(c.nonce);
    hashes[0].push_back(c.at ? std::optional<std::string_view>(*c.at) : std::nullopt);
    hashes[1].push_back(c.code ? std::optional<std::string_view>(*c.code) : std::nullopt);
  }
  const std::vector<const int64_t*> nums;

  PublicKey ed, rsa;
  ed.kind = PublicKey::Ed25519;
  ed.x = std::string(32, '\0');
  rsa.kind = PublicKey::RSA;
  rsa.n = std::string(256, '\xc5');
  rsa.e = 65537;
  std::string err;
  auto ks = NewStaticKeySet({ed, rsa}, &err);
  check(ks != nullptr, "static key set", err);
  if (!ks) return 1;
  auto v = NewValidator(ks.get(), &err);
  Expected ex;
  ex.SigningAlgorithms = {"EdDSA", "RS256", "RS384", "RS512"};
  ex.has_now = true;
  ex.now_unix_ns = 1611699344LL * 1000000000LL;
  ex.NotBeforeLeeway = 3600 * 1000000000LL;

  size_t want_host = 0, want_scanned = 0, host_values = 0;
  for (const Case& c : cases) {
    const bool verified = c.token.find('.') != std::string::npos;      // the stand-in accepts every signature
    want_host += verified && c.host;
    want_scanned += verified && !c.host;
  }
  CheckStats st;
  const int h0 = match_hash_stub_calls, a0 = match_args_stub_calls, d0 = hash_stub_calls;
  const auto rs = v->MatchBatchArgs(toks, ex, kReqs, strs, nums, &st, hashes);
  const auto cs = v->CheckBatch(toks, ex);
  check(match_hash_stub_calls == h0 + 1 && match_args_stub_calls == a0, "one jg_claims_match_hash call, no jg_claims_match_args call",
        std::to_string(match_hash_stub_calls - h0) + " / " + std::to_string(match_args_stub_calls - a0));
  check(match_hash_stub_refused == 0, "the ABI refused the host's call");
  check(hash_stub_calls == d0 + 1, "one jg_hash_batch call for the host path", std::to_string(hash_stub_calls - d0));
  check(st.host == want_host && st.scanned == want_scanned, "stats",
        std::to_string(st.scanned) + " scanned, " + std::to_string(st.host) + " host");
  for (size_t i = 0; i < n; ++i) {
    const std::string at = "token " + std::to_string(i);
    check(rs[i].ok == cs[i].ok && rs[i].err == cs[i].err, at + " differs from CheckBatch", rs[i].err + " / " + cs[i].err);
    check(rs[i].ok == cases[i].ok, at + " ok", rs[i].err);
    check(rs[i].bits == (cases[i].ok ? cases[i].bits : 0u), at + " bits",
          std::to_string(rs[i].bits) + " / " + std::to_string(cases[i].bits));
  }
  // the device hashed only values of scanned tokens under an RS alg; the host path hashed only its own
  check(match_hash_stub_sources > 0 && hash_stub_jobs > 0, "both paths hashed", std::to_string(match_hash_stub_sources) + " / " +
        std::to_string(hash_stub_jobs));
  for (size_t i = 0; i < n; ++i) host_values += cases[i].host ? (cases[i].at ? 1 : 0) + (cases[i].code ? 1 : 0) : 0;
  check((size_t)hash_stub_jobs <= host_values, "jg_hash_batch saw a value of a scanned token", std::to_string(hash_stub_jobs));
  // MatchVerdictsArgs holds the same rows
  {
    std::vector<uint8_t> ok(n, 0xee);
    std::vector<uint32_t> bits(n, 0xeeeeeeeeu);
    CheckStats s2;
    v->MatchVerdictsArgs(toks, ex, kReqs, strs, nums, ok.data(), bits.data(), &s2, hashes);
    for (size_t i = 0; i < n; ++i)
      check(ok[i] == (rs[i].ok ? 1 : 0) && bits[i] == rs[i].bits, "MatchVerdictsArgs token " + std::to_string(i));
    check(s2.scanned == st.scanned && s2.host == st.host, "MatchVerdictsArgs stats");
  }
  // an Expected per token
  {
    Expected late = ex;
    late.now_unix_ns = (1611699344LL + 7200) * 1000000000LL;
    const std::vector<Expected> es = {ex, late};
    std::vector<uint32_t> which(n);
    for (size_t i = 0; i < n; ++i) which[i] = (uint32_t)(i % 2);
    const auto each = v->MatchBatchArgsEach(toks, es, which, kReqs, strs, nums, nullptr, hashes);
    std::vector<uint8_t> ok(n);
    std::vector<uint32_t> bits(n);
    v->MatchVerdictsArgsEach(toks, es, which, kReqs, strs, nums, ok.data(), bits.data(), nullptr, hashes);
    const auto other = v->MatchBatchArgs(toks, late, kReqs, strs, nums, nullptr, hashes);
    size_t rejected = 0;
    for (size_t i = 0; i < n; ++i) {
      const MatchResult& alone = i % 2 ? other[i] : rs[i];
      check(each[i].ok == alone.ok && each[i].err == alone.err && each[i].bits == alone.bits, "MatchBatchArgsEach token " + std::to_string(i));
      check(ok[i] == (alone.ok ? 1 : 0) && bits[i] == alone.bits, "MatchVerdictsArgsEach token " + std::to_string(i));
      rejected += i % 2 && rs[i].ok && !alone.ok;
    }
    check(rejected >= 2, "the later clock rejects tokens", std::to_string(rejected));
  }
  // lists over the caps: every token takes the host path, the bits are the same
  {
    std::vector<HashColumn> three = hashes;
    three.push_back(hashes[0]);
    std::vector<std::vector<std::string_view>> strs3(3, strs[0]);
    std::vector<Require> longv = kReqs;
    longv.push_back(req({"nonce"}, R::Equals, 0, std::string(65, 'v')));
    for (int k = 0; k < 3; ++k) {
      CheckStats s2;
      const int c1 = match_hash_stub_calls;
      const auto r2 = k == 0   ? v->MatchBatchArgs(toks, ex, kReqs, strs, nums, &s2, three)
                      : k == 1 ? v->MatchBatchArgs(toks, ex, kReqs, strs3, nums, &s2, hashes)
                               : v->MatchBatchArgs(toks, ex, longv, strs, nums, &s2, hashes);
      check(match_hash_stub_calls == c1 && s2.scanned == 0 && s2.host == want_host + want_scanned,
            "a list over the caps reaches the ABI: " + std::to_string(k));
      for (size_t i = 0; i < n; ++i)
        check(r2[i].ok == rs[i].ok && (r2[i].bits & 31u) == rs[i].bits, "over the caps " + std::to_string(k) + " token " + std::to_string(i),
              std::to_string(r2[i].bits) + " / " + std::to_string(rs[i].bits));
    }
  }
  // IsString alone needs no column and still goes through the new entry; the old ops alone go through the old one
  {
    const int h1 = match_hash_stub_calls, a1 = match_args_stub_calls;
    const auto r2 = v->MatchBatchArgs(toks, ex, {kReqs[2], kReqs[4]}, {}, {});
    check(match_hash_stub_calls == h1 + 1 && match_args_stub_calls == a1, "IsString goes through jg_claims_match_hash");
    for (size_t i = 0; i < n; ++i)
      check(r2[i].bits == (((rs[i].bits >> 2) & 1u) | ((rs[i].bits >> 4) & 1u) << 1), "IsString alone: token " + std::to_string(i));
    const auto r3 = v->MatchBatchArgs(toks, ex, {kReqs[0]}, strs, nums);
    check(match_hash_stub_calls == h1 + 1 && match_args_stub_calls == a1 + 1, "the old ops go through jg_claims_match_args");
    for (size_t i = 0; i < n; ++i) check(r3[i].bits == (rs[i].bits & 1u), "EqualsArg alone: token " + std::to_string(i));
  }
  // a failed jg_hash_batch: the tokens that needed it get the scan's unavailable error, the others their rows
  {
    hash_stub_fail = 1;
    const auto r2 = v->MatchBatchArgs(toks, ex, kReqs, strs, nums, nullptr, hashes);
    hash_stub_fail = 0;
    size_t unavailable = 0;
    for (size_t i = 0; i < n; ++i) {
      if (r2[i].err.find("capjwt: claims scan unavailable: ") == 0) {
        ++unavailable;
        check(cases[i].host && !r2[i].ok && r2[i].bits == 0, "unavailable on a token that needed no host hash: " + std::to_string(i));
      } else {
        check(r2[i].ok == rs[i].ok && r2[i].bits == rs[i].bits && r2[i].err == rs[i].err, "failed hash: token " + std::to_string(i), r2[i].err);
      }
    }
    check(unavailable >= 1, "a failed jg_hash_batch surfaces", std::to_string(unavailable));
    const auto r3 = v->MatchBatchArgs(toks, ex, kReqs, strs, nums, nullptr, hashes);
    for (size_t i = 0; i < n; ++i) check(r3[i].ok == rs[i].ok && r3[i].bits == rs[i].bits, "after the failure: token " + std::to_string(i), r3[i].err);
  }
  // what no path takes
  {
    std::vector<HashColumn> shorter = hashes;
    shorter[1].pop_back();
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, kReqs, strs, nums, nullptr, shorter); }), "a short hash column throws");
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, {req({"a"}, R::HashOfArg, 2)}, strs, nums, nullptr, hashes); }),
          "a hash column index without a column throws");
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, {req({"a"}, R::HashOfArg, 0)}, strs, nums); }),
          "a hash column index without any column throws");
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, {req({"a"}, (R::Op)12)}, strs, nums, nullptr, hashes); }), "an unknown op throws");
    check(v->MatchBatchArgs({}, ex, kReqs, {{}}, {}, nullptr, {{}, {}}).empty(), "an empty batch");
    for (int op = 10; op <= 11; ++op) {
      check(throws([&] { (void)v->MatchBatch(toks, ex, {req({"a"}, (R::Op)op)}); }), "MatchBatch takes op " + std::to_string(op));
      check(throws([&] { (void)match_requires(json::Value{}, {req({"a"}, (R::Op)op)}, {}, {}); }),
            "match_requires without hash columns takes op " + std::to_string(op));
    }
    check(throws([&] { (void)match_requires(json::Value{}, {req({"a"}, R::HashOfArg, 1)}, {}, {}, {std::nullopt}); }),
          "match_requires: a hash column index without a column throws");
  }
  if (fails) return 1;
  std::printf("match hash: ok\n");
  return 0;
}
