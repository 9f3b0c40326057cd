// match.cpp -- the Match entries (Validator::MatchBatch and kin) without a GPU.
//
//   match ok       linked with match_stub.cpp: the bits of device-decided rows
//                  (the scan's masks) and of JG_CL_HOST rows (match_requires on the
//                  verified claims map) equal match_requires on ValidateBatch's
//                  claims map and the masks written below; ok / err are CheckBatch's,
//                  token for token; a rejected token carries no bits; a list the
//                  ABI refuses takes the host path for every token and gives the
//                  same bits; equal requirements share a predicate; MatchVerdicts
//                  holds MatchBatch's rows; the *Each forms hold each token to its
//                  own Expected; what no path takes throws
//   match nomatch  linked with match_stub.cpp built -DNO_MATCH: every token that
//                  reaches the scan gets "claims scan unavailable", CheckBatch and
//                  the Select entries by path still work
// Prints FAIL lines and exits 1 on a mismatch.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/host/cap_jwt.hpp"
#include "../../include/jg.h"

using namespace capjwt;

extern "C" int match_stub_calls;
extern "C" int paths_stub_calls;

static int fails = 0;
static void check(bool ok, const std::string& what, const std::string& got = "") {
  if (!ok) {
    std::printf("FAIL %s: %s\n", what.c_str(), got.c_str());
    ++fails;
  }
}
static bool has(const std::string& s, const char* sub) { return s.find(sub) != std::string::npos; }

static std::string token(const std::string& payload) {
  return b64url_encode(R"({"alg":"EdDSA","kid":"k1"})") + "." + b64url_encode(payload) + "." + std::string(86, 'A');
}

struct Case {
  std::string payload;
  bool ok;
  bool host;                                   // the scan leaves it to the host
  uint32_t want;                               // the mask under kReqs
};

using R = Require;
// bit 0 up
static const std::vector<Require> kReqs = {
    {{"realm_access", "roles"}, R::HasElement, "admin"}, {{"realm_access", "roles"}, R::HasElement, "dev"},
    {{"realm_access", "roles"}, R::Present, ""},         {{"realm_access"}, R::Present, ""},
    {{"scope"}, R::HasWord, "read"},                     {{"scope"}, R::HasWord, "read:all"},
    {{"scope"}, R::Equals, "read write"},                {{"azp"}, R::Equals, ""},
    {{"cnf", "jkt"}, R::Present, ""},                    {{"a", "b", "c", "d"}, R::HasElement, "a/b"},
    {{"aud"}, R::HasElement, "www.example.com"},         {{"aud"}, R::Equals, "www.example.com"}};

// the rows of one MatchBatch against ValidateBatch / CheckBatch and the cases' masks
static void compare(Validator& v, const std::vector<std::string_view>& toks, const Expected& ex,
                    const std::vector<Require>& reqs, const std::vector<Case>* cases, const std::string& tag,
                    CheckStats* st) {
  const auto rs = v.MatchBatch(toks, ex, reqs, st);
  const auto cs = v.CheckBatch(toks, ex);
  Results vs = v.ValidateBatch(toks, ex);
  check(rs.size() == toks.size(), tag + " size");
  for (size_t i = 0; i < rs.size(); ++i) {
    const std::string at = tag + " token " + std::to_string(i);
    check(rs[i].ok == cs[i].ok && rs[i].err == cs[i].err, at + " differs from CheckBatch", rs[i].err + " / " + cs[i].err);
    check(rs[i].ok == vs[i].ok && rs[i].err == vs[i].err, at + " differs from ValidateBatch", rs[i].err + " / " + vs[i].err);
    if (!rs[i].ok) {
      check(rs[i].bits == 0, at + ": a rejected token carries bits", std::to_string(rs[i].bits));
      continue;
    }
    const uint32_t m = match_requires(vs[i].claims, reqs);
    check(rs[i].bits == m, at + " differs from match_requires on ValidateBatch's map",
          std::to_string(rs[i].bits) + " / " + std::to_string(m));
    if (cases && i < cases->size()) check(rs[i].bits == (*cases)[i].want, at + " mask", std::to_string(rs[i].bits));
  }
}

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
  const std::string mode = argc > 1 ? argv[1] : "ok";
  const int64_t T0 = 1611699344;
  const std::vector<Case> cases = {
      // decided by the scan: the bits are the scan's masks
      {R"({"realm_access":{"roles":["admin","dev"]},"scope":"read write","azp":"","cnf":{"jkt":null},"aud":"www.example.com","exp":1611699944})",
       true, false, 0b1001'1101'1111},
      {R"({"exp":1611699944,"realm_access":{"roles":["admin"]},"realm_access":{},"scope":"thread read:all","aud":["x","www.example.com"]})",
       true, false, 0b0100'0010'1000},
      {R"({"exp":1611699944,"realm_access":{"roles":"admin"},"scope":["read"],"azp":null,"a":{"b":{"c":{"d":["a/b"]}}}})",
       true, false, 0b0010'0000'1100},
      {"{\"exp\":1611699944,\"realm_access\":{\"roles\":[\"adm\xc3\xadn\",[\"admin\"],\"dev\"]},\"scope\":\"r\xc3\xa9""ad  read\"}",
       true, false, 0b0000'0001'1110},
      {R"({"exp":1611699944})", true, false, 0},
      {R"({"exp":1611698344,"realm_access":{"roles":["admin"]}})", false, false, 0},
      // left to the host: the bits come from the verified claims map
      {R"({"realm_access":{"roles":["admin"]},"scope":"read write","a":{"b":{"c":{"d":["a\/b"]}}},"exp":1611699944})",
       true, true, 0b0010'0101'1101},
      {R"({"exp":1611699944,"EXP":1611699945,"realm_access":[],"cnf":{"jkt":1e3},"scope":"read:all"})", true, true, 0b0001'0010'1000},
      {R"({"sub":5,"exp":1611699944,"realm_access":{"roles":["admin"]}})", false, true, 0},
  };
  std::vector<std::string> store;
  for (const Case& c : cases) store.push_back(token(c.payload));
  store.push_back("not-a-jwt");
  std::vector<std::string_view> toks(store.begin(), store.end());
  const size_t nc = cases.size();

  PublicKey ed;
  ed.kind = PublicKey::Ed25519;
  ed.x = std::string(32, '\0');
  std::string err;
  auto ks = NewStaticKeySet({ed}, &err);
  check(ks != nullptr, "static key set", err);
  if (!ks) return 1;
  auto v = NewValidator(ks.get(), &err);
  Expected ex;
  ex.SigningAlgorithms = {"EdDSA"};
  ex.has_now = true;
  ex.now_unix_ns = T0 * 1000000000LL;
  ex.NotBeforeLeeway = 3600 * 1000000000LL;     // a token with exp alone: nbf defaults to an hour before it

  if (mode == "ok") {
    size_t want_host = 0;
    for (const Case& c : cases) want_host += c.host;
    CheckStats st;
    const int calls0 = match_stub_calls, pcalls0 = paths_stub_calls;
    compare(*v, toks, ex, kReqs, &cases, "twelve requirements", &st);
    check(match_stub_calls == calls0 + 1, "one jg_claims_match call per batch", std::to_string(match_stub_calls - calls0));
    check(paths_stub_calls == pcalls0, "no jg_claims_paths call");
    check(st.host == want_host && st.scanned == nc - want_host, "stats",
          std::to_string(st.scanned) + " scanned, " + std::to_string(st.host) + " host");
    // no requirement, one, and sixteen with repeats (twelve distinct): still the scan
    std::vector<Require> rep = kReqs;
    rep.insert(rep.end(), kReqs.begin(), kReqs.begin() + 4);
    rep[15].value = "ignored";                                    // Present does not read its value: still requirement 3
    for (const std::vector<Require>& reqs : {std::vector<Require>{}, std::vector<Require>{kReqs[4]}, rep}) {
      CheckStats s2;
      compare(*v, toks, ex, reqs, nullptr, std::to_string(reqs.size()) + " requirements", &s2);
      check(s2.scanned == st.scanned && s2.host == st.host, std::to_string(reqs.size()) + " requirements: stats");
    }
    {
      const auto rs = v->MatchBatch(toks, ex, rep);
      for (size_t i = 0; i < nc; ++i)
        if (cases[i].ok)
          check(rs[i].bits == (cases[i].want | (cases[i].want & 0xfu) << 12),
                "repeats: token " + std::to_string(i), std::to_string(rs[i].bits));
    }
    // a list the ABI refuses: every token takes the host path, the bits are the same
    std::vector<std::vector<Require>> refused(8, kReqs);
    for (const char* nm : {"p6", "p7", "p8"}) refused[0].push_back({{nm}, R::Present, ""});        // nine distinct paths
    refused[1].push_back({{"a", "b", "c", "d", "e"}, R::Present, ""});                            // five components
    refused[2].push_back({{"scope"}, R::Equals, std::string(65, 'v')});                           // a value over 64 bytes
    refused[3].push_back({{"realm_access", "roles"}, R::HasElement, "adm\xc3\xadn"});             // non-ASCII bytes
    refused[4].push_back({{"scope"}, R::HasWord, "read write"});                                  // a space in a word
    refused[5].push_back({{"scope"}, R::HasWord, ""});                                            // an empty word
    refused[6].push_back({{"realm_access", "roles"}, R::HasElement, ""});                         // an empty element
    refused[7].push_back({{"cnf", "x5t\"S256"}, R::Present, ""});                                 // a quote in a component
    for (size_t k = 0; k < refused.size(); ++k) {
      CheckStats s2;
      const int c1 = match_stub_calls;
      compare(*v, toks, ex, refused[k], nullptr, "refused list " + std::to_string(k), &s2);
      check(match_stub_calls == c1, "refused list " + std::to_string(k) + " reaches jg_claims_match");
      check(s2.scanned == 0 && s2.host == nc, "refused list " + std::to_string(k) + ": stats",
            std::to_string(s2.scanned) + " scanned, " + std::to_string(s2.host) + " host");
      const auto rs = v->MatchBatch(toks, ex, refused[k]);
      for (size_t i = 0; i < nc; ++i)
        if (cases[i].ok) check((rs[i].bits & 0xfffu) == cases[i].want, "refused list " + std::to_string(k) + " token " + std::to_string(i));
    }
    check(v->MatchBatch(toks, ex, refused[3])[3].bits >> 12 == 1, "a non-ASCII value matches on the host path");
    // MatchVerdicts holds MatchBatch's rows
    {
      const auto rs = v->MatchBatch(toks, ex, kReqs);
      std::vector<uint8_t> ok(toks.size(), 0xee);
      std::vector<uint32_t> bits(toks.size(), 0xeeeeeeeeu);
      CheckStats s2;
      v->MatchVerdicts(toks, ex, kReqs, ok.data(), bits.data(), &s2);
      for (size_t i = 0; i < toks.size(); ++i)
        check(ok[i] == (rs[i].ok ? 1 : 0) && bits[i] == rs[i].bits, "MatchVerdicts token " + std::to_string(i));
      check(s2.scanned == st.scanned && s2.host == st.host, "MatchVerdicts stats");
    }
    // an Expected per token: each row is its own Expected's
    {
      Expected late = ex;
      late.now_unix_ns = (T0 + 7200) * 1000000000LL;
      Expected aud = ex;
      aud.Audiences = {"www.example.com"};
      const std::vector<Expected> es = {ex, late, aud};
      std::vector<uint32_t> which(toks.size());
      for (size_t i = 0; i < which.size(); ++i) which[i] = (uint32_t)(i % 3);
      const int c1 = match_stub_calls;
      const auto each = v->MatchBatchEach(toks, es, which, kReqs);
      check(match_stub_calls == c1 + 1, "one jg_claims_match call for the *Each batch");
      std::vector<uint8_t> ok(toks.size());
      std::vector<uint32_t> bits(toks.size());
      v->MatchVerdictsEach(toks, es, which, kReqs, ok.data(), bits.data());
      size_t rejected = 0;
      for (size_t p = 0; p < es.size(); ++p) {
        const auto alone = v->MatchBatch(toks, es[p], kReqs);
        for (size_t i = p; i < toks.size(); i += 3) {
          check(each[i].ok == alone[i].ok && each[i].err == alone[i].err && each[i].bits == alone[i].bits,
                "MatchBatchEach token " + std::to_string(i), each[i].err + " / " + alone[i].err);
          check(ok[i] == (alone[i].ok ? 1 : 0) && bits[i] == alone[i].bits, "MatchVerdictsEach token " + std::to_string(i));
          rejected += !alone[i].ok && cases.size() > i && cases[i].ok;
        }
      }
      check(rejected >= 2, "the other Expecteds reject tokens the first accepts", std::to_string(rejected));
    }
    // what no path takes
    std::vector<Require> seventeen(17, Require{{"a"}, R::Present, ""});
    for (size_t k = 0; k < seventeen.size(); ++k) seventeen[k].path[0] += std::to_string(k);
    check(throws([&] { (void)v->MatchBatch(toks, ex, seventeen); }), "seventeen requirements throw");
    check(throws([&] { (void)match_requires(json::Value{}, seventeen); }), "seventeen requirements throw on the host path");
    check(throws([&] { (void)v->MatchBatch(toks, ex, {Require{{}, R::Present, ""}}); }), "a path without components throws");
    check(throws([&] { (void)v->MatchBatch(toks, ex, {Require{{"a", std::string("b\0c", 3)}, R::Present, ""}}); }),
          "a NUL in a component throws");
    check(throws([&] { (void)v->MatchBatch(toks, ex, {Require{{"a"}, R::Equals, std::string("b\0c", 3)}}); }),
          "a NUL in a value throws");
    check(throws([&] { (void)v->MatchBatch(toks, ex, {Require{{"a"}, (R::Op)9, ""}}); }), "an unknown op throws");
    check(v->MatchBatch({}, ex, kReqs).empty(), "an empty batch");
  } else if (mode == "nomatch") {
    const auto rs = v->MatchBatch(toks, ex, kReqs);
    for (size_t i = 0; i < nc; ++i)
      check(!rs[i].ok && rs[i].bits == 0 && has(rs[i].err, "claims scan unavailable") && has(rs[i].err, "jg_claims_match"),
            "nomatch token " + std::to_string(i), rs[i].err);
    // the entries beside it still work with the same library
    const auto cs = v->CheckBatch(toks, ex);
    for (size_t i = 0; i < nc; ++i) check(cs[i].ok == cases[i].ok, "nomatch CheckBatch token " + std::to_string(i), cs[i].err);
    const auto ss = v->SelectBatch(toks, ex, ClaimPaths{{{"realm_access", "roles"}}});
    for (size_t i = 0; i < nc; ++i) check(ss[i].ok == cases[i].ok, "nomatch SelectBatch token " + std::to_string(i), ss[i].err);
    // a list the scan would not take never needed the entry
    std::vector<Require> host_only = kReqs;
    host_only.push_back({{"scope"}, R::HasWord, ""});
    const auto hs = v->MatchBatch(toks, ex, host_only);
    for (size_t i = 0; i < nc; ++i)
      check(hs[i].ok == cases[i].ok && (hs[i].bits & 0xfffu) == cases[i].want, "nomatch host-only list token " + std::to_string(i), hs[i].err);
  } else {
    std::printf("unknown mode %s\n", mode.c_str());
    return 2;
  }
  if (fails) return 1;
  std::printf("match %s: ok\n", mode.c_str());
  return 0;
}
