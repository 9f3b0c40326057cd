// match_args.cpp -- the MatchArgs entries (Validator::MatchBatchArgs and kin)
// without a GPU, linked with match_args_stub.cpp.
//
// The bits of device-decided rows (the scan's masks) and of host-path rows
// (match_requires with the token's operands on the verified claims map) equal
// match_requires on ValidateBatch's claims map and the masks written below; ok /
// err are CheckBatch's, token for token; a token whose own operand the scan
// refuses takes the host path and no refused operand reaches the ABI; a token
// with a fractional or 16-digit number under a numeric requirement is left to
// the host by the scan; a list over the caps sends every token to the host path
// and gives the same bits; MatchVerdictsArgs holds MatchBatchArgs' rows; the
// *Each forms hold each token to its own Expected; what no path takes throws;
// the MatchBatch family keeps refusing the new ops.
// Prints FAIL lines and exits 1 on a mismatch.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/host/cap_jwt.hpp"
#include "../../include/jg.h"

using namespace capjwt;

extern "C" int match_stub_calls;
extern "C" int match_args_stub_calls;
extern "C" int match_args_stub_refused;

static int fails = 0;
static void check(bool ok, const std::string& what, const std::string& got = "") {
  if (!ok) {
    std::printf("FAIL %s: %s\n", what.c_str(), got.c_str());
    ++fails;
  }
}

static std::string token(const std::string& payload) {
  return b64url_encode(R"({"alg":"EdDSA","kid":"k1"})") + "." + b64url_encode(payload) + "." + std::string(86, 'A');
}

struct Case {
  std::string payload;
  std::string nonce, jkt;                      // string columns 0 and 1
  int64_t n0, n1;                              // number columns 0 and 1
  bool ok;
  bool host;                                   // the token takes the host path
  uint32_t want;                               // the mask under kReqs
};

using R = Require;
static Require req(ClaimPath path, R::Op op, std::string value = "", int64_t bound = 0, uint32_t column = 0) {
  Require r;
  r.path = std::move(path);
  r.op = op;
  r.value = std::move(value);
  r.bound = bound;
  r.column = column;
  return r;
}
// bit 0 up
static const std::vector<Require> kReqs = {
    req({"nonce"}, R::EqualsArg, "", 0, 0),          req({"auth_time"}, R::AtLeastArg, "", 0, 0),
    req({"cnf", "jkt"}, R::EqualsArg, "", 0, 1),     req({"auth_time"}, R::AtMostArg, "", 0, 1),
    req({"auth_time"}, R::AtLeast, "", 1000),        req({"auth_time"}, R::AtMost, "", 1611699344),
    req({"scope"}, R::HasWord, "read"),              req({"nonce"}, R::Equals, "abc"),
    req({"nonce"}, R::Present),                      req({"cnf", "jkt"}, R::EqualsArg, "", 0, 0)};

struct Cols {
  std::vector<std::vector<std::string_view>> strs;
  std::vector<std::vector<int64_t>> numv;
  std::vector<const int64_t*> nums;
};
static Cols columns(const std::vector<Case>& cases, size_t n) {
  Cols c;
  c.strs.assign(2, std::vector<std::string_view>(n));
  c.numv.assign(2, std::vector<int64_t>(n, 0));
  for (size_t i = 0; i < cases.size(); ++i) {
    c.strs[0][i] = cases[i].nonce;
    c.strs[1][i] = cases[i].jkt;
    c.numv[0][i] = cases[i].n0;
    c.numv[1][i] = cases[i].n1;
  }
  for (auto& v : c.numv) c.nums.push_back(v.data());
  return c;
}

static void compare(Validator& v, const std::vector<std::string_view>& toks, const Expected& ex,
                    const std::vector<Require>& reqs, const Cols& cols, const std::vector<Case>* cases,
                    const std::string& tag, CheckStats* st) {
  const auto rs = v.MatchBatchArgs(toks, ex, reqs, cols.strs, cols.nums, st);
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
    std::vector<std::string_view> s;
    std::vector<int64_t> n;
    for (const auto& col : cols.strs) s.push_back(col[i]);
    for (const int64_t* col : cols.nums) n.push_back(col[i]);
    const uint32_t m = match_requires(vs[i].claims, reqs, s, n);
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

int main() {
  const int64_t T0 = 1611699344;
  const std::string jkt = "0ZcOCORZNYy-DWpqq30jZyJGHTN0d2HglBV3uiguA4I";
  const std::vector<Case> cases = {
      // decided by the scan
      {R"({"nonce":"n-0S6_WzA2Mj","auth_time":1611699300,"cnf":{"jkt":")" + jkt + R"("},"scope":"openid read","exp":1611699944})",
       "n-0S6_WzA2Mj", jkt, 1611699284, 1611699344, true, false, 0b01'0111'1111},
      {R"({"nonce":"n-0S6_WzA2Mj","auth_time":1611699200,"cnf":{"jkt":")" + jkt + R"("},"scope":"openid","exp":1611699944})",
       "n-0S6_WzA2Mk", "other", 1611699284, 1611699199, true, false, 0b01'0011'0000},
      {R"({"nonce":"abc","auth_time":5,"cnf":{"jkt":"abc"},"exp":1611699944})", "abc", "abc", 5, 5, true, false, 0b11'1010'1111},
      {R"({"nonce":"","auth_time":-0,"exp":1611699944})", "", "", 0, 0, true, false, 0b01'0010'1011},
      {R"({"nonce":["abc"],"auth_time":"1000","cnf":{"jkt":7},"exp":1611699944})", "abc", "7", 1000, 1000, true, false, 0b01'0000'0000},
      {R"({"exp":1611699944})", "", "", INT64_MIN, INT64_MAX, true, false, 0},
      {R"({"nonce":"abc","auth_time":999999999999999,"exp":1611699944})", "abc", "", INT64_MAX, INT64_MIN, true, false, 0b01'1001'0001},
      {R"({"exp":1611698344,"nonce":"abc"})", "abc", "", 0, 0, false, false, 0},
      // the scan leaves these to the host: a number it does not decide, an escape
      {R"({"nonce":"abc","auth_time":1611699300.5,"exp":1611699944})", "abc", "", 1611699300, 1611699301, true, true, 0b01'1011'1011},
      {R"({"nonce":"abc","auth_time":1000000000000000,"exp":1611699944})", "abd", "", 1000000000000000, 999999999999999, true, true,
       0b01'1001'0010},
      {R"({"nonce":"abc","auth_time":1e3,"cnf":{"jkt":"k"},"exp":1611699944})", "abc", "k", 1000, 1000, true, true, 0b01'1011'1111},
      {R"({"nonce":"abc","auth_time":0.5,"auth_time":7,"exp":1611699944})", "abc", "", 7, 7, true, true, 0b01'1010'1011},
      // an operand the scan refuses: the token takes the host path, and the host compares the bytes
      {"{\"nonce\":\"n\xc3\xb8nce\",\"auth_time\":5,\"exp\":1611699944}", "n\xc3\xb8nce", "", 5, 5, true, true, 0b01'0010'1011},
      {R"({"nonce":")" + std::string(70, 'v') + R"(","exp":1611699944})", std::string(70, 'v'), "", 0, 0, true, true, 0b01'0000'0001},
      {R"({"nonce":"say \"hi\"","cnf":{"jkt":"a\\b"},"exp":1611699944})", "say \"hi\"", "a\\b", 0, 0, true, true, 0b01'0000'0101},
      {R"({"nonce":"abc","cnf":{"jkt":"tab"},"exp":1611699944})", "abc", "ta\tb", 0, 0, true, true, 0b01'1000'0001},
  };
  std::vector<std::string> store;
  for (const Case& c : cases) store.push_back(token(c.payload));
  store.push_back("not-a-jwt");
  std::vector<std::string_view> toks(store.begin(), store.end());
  const size_t nc = cases.size();
  const Cols cols = columns(cases, toks.size());

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

  size_t want_host = 0;
  for (const Case& c : cases) want_host += c.host;
  CheckStats st;
  const int calls0 = match_args_stub_calls, old0 = match_stub_calls;
  compare(*v, toks, ex, kReqs, cols, &cases, "ten requirements", &st);
  check(match_args_stub_calls == calls0 + 1, "one jg_claims_match_args call per batch",
        std::to_string(match_args_stub_calls - calls0));
  check(match_stub_calls == old0, "no jg_claims_match call");
  check(match_args_stub_refused == 0, "a refused operand reached the ABI");
  check(st.host == want_host && st.scanned == nc - want_host, "stats",
        std::to_string(st.scanned) + " scanned, " + std::to_string(st.host) + " host");
  // no requirement; the old ops alone; repeats share a predicate
  std::vector<Require> rep = kReqs;
  rep.insert(rep.end(), kReqs.begin(), kReqs.begin() + 6);
  for (const std::vector<Require>& reqs : {std::vector<Require>{}, std::vector<Require>{kReqs[6], kReqs[7]}, rep}) {
    CheckStats s2;
    compare(*v, toks, ex, reqs, cols, nullptr, std::to_string(reqs.size()) + " requirements", &s2);
    if (reqs.size() == 16) {
      const auto rs = v->MatchBatchArgs(toks, ex, reqs, cols.strs, cols.nums);
      for (size_t i = 0; i < nc; ++i)
        if (cases[i].ok)
          check(rs[i].bits == (cases[i].want | (cases[i].want & 0x3fu) << 10), "repeats: token " + std::to_string(i),
                std::to_string(rs[i].bits));
    }
  }
  // without a numeric requirement the fractional tokens are the scan's again
  {
    CheckStats s2;
    compare(*v, toks, ex, {kReqs[0], kReqs[2], kReqs[8]}, cols, nullptr, "no numeric requirement", &s2);
    check(s2.host == want_host - 3, "no numeric requirement: stats", std::to_string(s2.host));
  }
  check(match_args_stub_refused == 0, "a refused operand reached the ABI");
  // lists over the caps: every token takes the host path, the bits are the same
  {
    std::vector<std::vector<Require>> refused(3, kReqs);
    for (const char* nm : {"p4", "p5", "p6", "p7", "p8"}) refused[0].push_back(req({nm}, R::Present));   // nine distinct paths
    refused[1].push_back(req({"a", "b", "c", "d", "e"}, R::AtLeast, "", 1));                             // five components
    refused[2].push_back(req({"scope"}, R::Equals, std::string(65, 'v')));                               // a value over 64 bytes
    for (size_t k = 0; k < refused.size(); ++k) {
      CheckStats s2;
      const int c1 = match_args_stub_calls;
      compare(*v, toks, ex, refused[k], cols, nullptr, "refused list " + std::to_string(k), &s2);
      check(match_args_stub_calls == c1, "refused list " + std::to_string(k) + " reaches the ABI");
      check(s2.scanned == 0 && s2.host == nc, "refused list " + std::to_string(k) + ": stats");
      const auto rs = v->MatchBatchArgs(toks, ex, refused[k], cols.strs, cols.nums);
      for (size_t i = 0; i < nc; ++i)
        if (cases[i].ok) check((rs[i].bits & 0x3ffu) == cases[i].want, "refused list " + std::to_string(k) + " token " + std::to_string(i));
    }
    // five string columns: over JG_MAX_ARGS
    Cols five = cols;
    for (int k = 0; k < 3; ++k) five.strs.push_back(cols.strs[0]);
    std::vector<Require> reqs5 = kReqs;
    reqs5.push_back(req({"nonce"}, R::EqualsArg, "", 0, 4));
    CheckStats s2;
    const int c1 = match_args_stub_calls;
    compare(*v, toks, ex, reqs5, five, nullptr, "five columns", &s2);
    check(match_args_stub_calls == c1 && s2.scanned == 0 && s2.host == nc, "five columns take the host path");
    const auto rs = v->MatchBatchArgs(toks, ex, reqs5, five.strs, five.nums);
    for (size_t i = 0; i < nc; ++i)
      if (cases[i].ok) check(rs[i].bits == (cases[i].want | (cases[i].want & 1u) << 10), "five columns token " + std::to_string(i));
  }
  // MatchVerdictsArgs holds MatchBatchArgs' rows
  {
    const auto rs = v->MatchBatchArgs(toks, ex, kReqs, cols.strs, cols.nums);
    std::vector<uint8_t> ok(toks.size(), 0xee);
    std::vector<uint32_t> bits(toks.size(), 0xeeeeeeeeu);
    CheckStats s2;
    v->MatchVerdictsArgs(toks, ex, kReqs, cols.strs, cols.nums, ok.data(), bits.data(), &s2);
    for (size_t i = 0; i < toks.size(); ++i)
      check(ok[i] == (rs[i].ok ? 1 : 0) && bits[i] == rs[i].bits, "MatchVerdictsArgs token " + std::to_string(i));
    check(s2.scanned == st.scanned && s2.host == st.host, "MatchVerdictsArgs stats");
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
    const int c1 = match_args_stub_calls;
    const auto each = v->MatchBatchArgsEach(toks, es, which, kReqs, cols.strs, cols.nums);
    check(match_args_stub_calls == c1 + 1, "one jg_claims_match_args call for the *Each batch");
    std::vector<uint8_t> ok(toks.size());
    std::vector<uint32_t> bits(toks.size());
    v->MatchVerdictsArgsEach(toks, es, which, kReqs, cols.strs, cols.nums, ok.data(), bits.data());
    size_t rejected = 0;
    for (size_t p = 0; p < es.size(); ++p) {
      const auto alone = v->MatchBatchArgs(toks, es[p], kReqs, cols.strs, cols.nums);
      for (size_t i = p; i < toks.size(); i += 3) {
        check(each[i].ok == alone[i].ok && each[i].err == alone[i].err && each[i].bits == alone[i].bits,
              "MatchBatchArgsEach token " + std::to_string(i), each[i].err + " / " + alone[i].err);
        check(ok[i] == (alone[i].ok ? 1 : 0) && bits[i] == alone[i].bits, "MatchVerdictsArgsEach token " + std::to_string(i));
        rejected += !alone[i].ok && cases.size() > i && cases[i].ok;
      }
    }
    check(rejected >= 2, "the other Expecteds reject tokens the first accepts", std::to_string(rejected));
  }
  check(match_args_stub_refused == 0, "a refused operand reached the ABI");
  // what no path takes
  {
    std::vector<Require> seventeen(17, req({"a"}, R::AtLeast, "", 0));
    for (size_t k = 0; k < seventeen.size(); ++k) seventeen[k].bound = (int64_t)k;
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, seventeen, cols.strs, cols.nums); }), "seventeen requirements throw");
    Cols shorter = cols;
    shorter.strs[1].pop_back();
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, kReqs, shorter.strs, cols.nums); }), "a short column throws");
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, {req({"a"}, R::EqualsArg, "", 0, 2)}, cols.strs, cols.nums); }),
          "a string column index without a column throws");
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, {req({"a"}, R::AtMostArg, "", 0, 2)}, cols.strs, cols.nums); }),
          "a number column index without a column throws");
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, {req({"a"}, R::AtLeastArg, "", 0, 0)}, cols.strs, {}); }),
          "a number column index without any column throws");
    Cols nul = cols;
    const std::string with_nul("a\0b", 3);
    nul.strs[0][2] = with_nul;
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, kReqs, nul.strs, cols.nums); }), "a NUL in an operand throws");
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, {req({"a"}, (R::Op)10)}, cols.strs, cols.nums); }), "an unknown op throws");
    check(throws([&] { (void)v->MatchBatchArgs(toks, ex, {req({}, R::AtLeast)}, cols.strs, cols.nums); }), "a path without components throws");
    check(throws([&] { (void)match_requires(json::Value{}, {req({"a"}, R::EqualsArg, "", 0, 1)}, {"x"}, {}); }),
          "match_requires: a column index without a column throws");
    check(v->MatchBatchArgs({}, ex, kReqs, {{}, {}}, {nullptr, nullptr}).empty(), "an empty batch");
    check(v->MatchBatchArgs({}, ex, {req({"a"}, R::AtLeast, "", 1)}, {}, {}).empty(), "an empty batch without columns");
    // the MatchBatch family keeps refusing the new ops
    for (int op = 5; op <= 9; ++op) {
      check(throws([&] { (void)v->MatchBatch(toks, ex, {req({"a"}, (R::Op)op)}); }), "MatchBatch takes op " + std::to_string(op));
      check(throws([&] { (void)match_requires(json::Value{}, {req({"a"}, (R::Op)op)}); }),
            "match_requires without operands takes op " + std::to_string(op));
    }
  }
  if (fails) return 1;
  std::printf("match args: ok\n");
  return 0;
}
