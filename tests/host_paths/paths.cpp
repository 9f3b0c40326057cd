// paths.cpp -- the Select entries by path (Validator::SelectBatch and kin with
// ClaimPaths) without a GPU.
//
//   paths ok       linked with paths_stub.cpp: the values of device-decided rows
//                  (from the scan's jg_selected records) and of JG_CL_HOST rows
//                  (from the verified claims map) equal the walk of
//                  ValidateBatch's claims map along each path and the JSON written
//                  below; ok / err are CheckBatch's, token for token; a path list
//                  the ABI refuses takes the host path for every token and gives
//                  the same values; one-component paths give what the names give;
//                  SelectCols holds SelectBatch's rows; the *Each forms hold each
//                  token to its own Expected
//   paths nopaths  linked with paths_stub.cpp built -DNO_PATHS: every token that
//                  reaches the scan gets "claims scan unavailable", the entries by
//                  name still work
// Prints FAIL lines and exits 1 on a mismatch.
#include <cstdio>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/host/cap_jwt.hpp"
#include "../../include/jg.h"

using namespace capjwt;

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

static const char* kAbsent = "<absent>";
static std::string show(const std::optional<json::Value>& v) { return v ? json::marshal(*v) : std::string(kAbsent); }
static std::string show(const json::Value* v) { return v ? json::marshal(*v) : std::string(kAbsent); }
static std::string name_of(const ClaimPath& p) {
  std::string s;
  for (const std::string& c : p) s += "/" + c;
  return s;
}

// the claims map walked along the path, as a caller of ValidateBatch would
static const json::Value* walk(const json::Value& all, const ClaimPath& path) {
  const json::Value* cur = &all;
  for (const std::string& c : path) {
    if (cur->kind != json::Value::Object) return nullptr;
    cur = cur->get(c);
    if (!cur) return nullptr;
  }
  return cur;
}

struct Case {
  std::string payload;
  bool ok;
  bool host;                                   // the scan leaves it to the host
  std::vector<std::string> want;               // json::marshal of the value per path of kPaths, or kAbsent
};

static const ClaimPaths kPaths = {{{"realm_access", "roles"}, {"realm_access", "groups"}, {"realm_access"},
                                   {"cnf", "jkt"}, {"a", "b", "c", "d"}, {"scope"}}};

// the rows of one SelectBatch against ValidateBatch / CheckBatch and the cases' JSON
static void compare(Validator& v, const std::vector<std::string_view>& toks, const Expected& ex, const ClaimPaths& paths,
                    const std::vector<Case>* cases, const std::string& tag, CheckStats* st) {
  const auto rs = v.SelectBatch(toks, ex, paths, st);
  const auto cs = v.CheckBatch(toks, ex);
  Results vs = v.ValidateBatch(toks, ex);
  check(rs.size() == toks.size(), tag + " size");
  for (size_t i = 0; i < rs.size(); ++i) {
    const std::string at = tag + " token " + std::to_string(i);
    check(rs[i].ok == cs[i].ok && rs[i].err == cs[i].err, at + " differs from CheckBatch", rs[i].err + " / " + cs[i].err);
    check(rs[i].ok == vs[i].ok && rs[i].err == vs[i].err, at + " differs from ValidateBatch", rs[i].err + " / " + vs[i].err);
    if (!rs[i].ok) {
      check(rs[i].values.empty(), at + ": a rejected token carries values");
      continue;
    }
    check(rs[i].values.size() == paths.paths.size(), at + " values size");
    for (size_t k = 0; k < paths.paths.size() && k < rs[i].values.size(); ++k) {
      const std::string got = show(rs[i].values[k]), nm = name_of(paths.paths[k]);
      const json::Value* m = walk(vs[i].claims, paths.paths[k]);
      check(got == show(m), at + " " + nm + " differs from the walk of ValidateBatch's map", got + " / " + show(m));
      if (m && rs[i].values[k])
        check(m->kind == rs[i].values[k]->kind && std::memcmp(&m->num, &rs[i].values[k]->num, 8) == 0,
              at + " " + nm + " kind / float bits");
      if (cases && i < cases->size()) check(got == (*cases)[i].want[k], at + " " + nm, got);
    }
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "ok";
  const int64_t T0 = 1611699344;
  const std::string A = kAbsent;
  const std::vector<Case> cases = {
      // decided by the scan: the values come from the records
      {R"({"realm_access":{"roles":["admin","dev"],"groups":"/g"},"cnf":{"jkt":"0Zc"},"a":{"b":{"c":{"d":1.5}}},"scope":"r w","exp":1611699944})",
       true, false, {"[\"admin\",\"dev\"]", "\"/g\"", "{\"groups\":\"/g\",\"roles\":[\"admin\",\"dev\"]}", "\"0Zc\"", "1.5", "\"r w\""}},
      {R"({"exp":1611699944,"realm_access":{"roles":[1]},"realm_access":{"groups":null},"cnf":[{"jkt":1}],"a":{"b":{"c":{"d":{"e":[ ]}}}}})",
       true, false, {A, "null", "{\"groups\":null}", A, "{\"e\":[]}", A}},
      {R"({"exp":1611699944,"realm_access":5,"cnf":{"jkt":"first","jkt":{"k":true}},"x":{"realm_access":{"roles":1}},"a":{"b":{"c":[{"d":1}]}}})",
       true, false, {A, A, "5", "{\"k\":true}", A, A}},
      {"{\"exp\":1611699944,\"realm_access\":{\"r\xc3\xb4les\":1,\"roles\":\"J\xc3\xbcrgen\"},\"cnf\":{\"jkt\":12345678901234567}}",
       true, false, {"\"J\xc3\xbcrgen\"", A, "{\"roles\":\"J\xc3\xbcrgen\",\"r\xc3\xb4les\":1}", "12345678901234568", A, A}},
      {R"({"exp":1611699944})", true, false, {A, A, A, A, A, A}},
      {R"({"exp":1611698344,"realm_access":{"roles":["late"]}})", false, false, {}},
      // left to the host: the values come from the verified claims map
      {R"({"realm_access":{"roles":["a\/b"],"groups":[ 1 , { "k" : [ ] } ]},"cnf":{"jkt":1e3},"a":{"b":{"c":{"d":false}}},"exp":1611699944})",
       true, true, {"[\"a/b\"]", "[1,{\"k\":[]}]", "{\"groups\":[1,{\"k\":[]}],\"roles\":[\"a/b\"]}", "1000", "false", A}},
      {R"({"exp":1611699944,"EXP":1611699945,"realm_access":{"roles":1},"realm_access":[],"cnf":{"jkt":null},"scope":{"z":1,"a":2}})",
       true, true, {A, A, "[]", "null", A, "{\"a\":2,\"z\":1}"}},
      {R"({"sub":5,"exp":1611699944,"realm_access":{"roles":["x"]}})", false, true, {}},
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
    const int calls0 = paths_stub_calls;
    compare(*v, toks, ex, kPaths, &cases, "six paths", &st);
    check(paths_stub_calls == calls0 + 1, "one jg_claims_paths call per batch", std::to_string(paths_stub_calls - calls0));
    check(st.host == want_host && st.scanned == nc - want_host, "stats",
          std::to_string(st.scanned) + " scanned, " + std::to_string(st.host) + " host");
    // a list of names makes the calls it made before
    {
      const int c1 = paths_stub_calls;
      (void)v->SelectBatch(toks, ex, {"scope", "cnf"});
      check(paths_stub_calls == c1, "names do not reach jg_claims_paths");
    }
    // no path, one path, eight paths of every length: still the scan
    const std::vector<ClaimPaths> lists = {
        ClaimPaths{},
        ClaimPaths{{{"cnf", "jkt"}}},
        ClaimPaths{{{"a"}, {"a", "b"}, {"a", "b", "c"}, {"a", "b", "c", "d"}, {"realm_access", "roles"},
                    {"realm_access", "role"}, {"cnf", "jkt", "k"}, {"scope", "a"}}},
    };
    for (const ClaimPaths& paths : lists) {
      CheckStats s2;
      compare(*v, toks, ex, paths, nullptr, std::to_string(paths.paths.size()) + " paths", &s2);
      check(s2.scanned == st.scanned && s2.host == st.host, std::to_string(paths.paths.size()) + " paths: stats");
    }
    // equal paths share a slot: eight distinct paths and repeats are still the scan
    {
      ClaimPaths paths = lists[2];
      paths.paths.push_back({"a", "b"});
      paths.paths.insert(paths.paths.begin(), {"cnf", "jkt", "k"});
      CheckStats s2;
      compare(*v, toks, ex, paths, nullptr, "repeated paths", &s2);
      check(s2.scanned == st.scanned, "repeated paths: stats");
    }
    // one-component paths give what the names give
    {
      const std::vector<std::string> names = {"scope", "cnf", "realm_access", "missing"};
      ClaimPaths paths;
      for (const std::string& nm : names) paths.paths.push_back({nm});
      const auto a = v->SelectBatch(toks, ex, names), b = v->SelectBatch(toks, ex, paths);
      for (size_t i = 0; i < a.size(); ++i) {
        check(a[i].ok == b[i].ok && a[i].err == b[i].err && a[i].values.size() == b[i].values.size(),
              "one component: token " + std::to_string(i));
        for (size_t k = 0; k < a[i].values.size() && k < b[i].values.size(); ++k)
          check(show(a[i].values[k]) == show(b[i].values[k]), "one component: value", show(b[i].values[k]));
      }
    }
    // a path list the ABI refuses: every token takes the host path, the values are the same
    std::vector<ClaimPaths> refused(6, kPaths);
    refused[0].paths.insert(refused[0].paths.end(), {{"p7"}, {"p8"}, {"p9", "x"}});      // nine distinct paths
    refused[1].paths.push_back({"a", "b", "c", "d", "e"});                                // five components
    refused[2].paths.push_back({"realm_access", std::string(65, 'L')});                   // a component over 64 bytes
    refused[3].paths.push_back({"realm_access", "r\xc3\xb4les"});                         // non-ASCII bytes
    refused[4].paths.push_back({"cnf", "x5t\"S256"});                                     // a quote
    refused[5].paths.push_back({"cnf", ""});                                              // an empty component
    for (size_t r = 0; r < refused.size(); ++r) {
      CheckStats s2;
      const int c1 = paths_stub_calls;
      compare(*v, toks, ex, refused[r], nullptr, "refused list " + std::to_string(r), &s2);
      check(s2.scanned == 0 && s2.host == nc, "refused list " + std::to_string(r) + ": stats",
            std::to_string(s2.scanned) + " scanned, " + std::to_string(s2.host) + " host");
      check(paths_stub_calls == c1, "refused list " + std::to_string(r) + ": no scan call");
    }
    {
      const auto rs = v->SelectBatch(toks, ex, refused[3]);
      check(rs[3].ok && show(rs[3].values[6]) == "1" && show(rs[0].values[0]) == "[\"admin\",\"dev\"]",
            "refused list: values from the map", show(rs[3].values[6]));
    }
    for (const ClaimPaths& bad : {ClaimPaths{{{"scope"}, {}}}, ClaimPaths{{{"cnf", std::string("a\0b", 3)}}}}) {
      bool threw = false;
      try {
        v->SelectBatch(toks, ex, bad);
      } catch (const std::invalid_argument&) {
        threw = true;
      }
      check(threw, "a path without components or with a NUL byte is refused with an exception");
    }
    check(v->SelectBatch({}, ex, kPaths).empty(), "empty batch");
    // the alg header check stays on the host and comes ahead of any claim error
    Expected ex3 = ex;
    ex3.SigningAlgorithms = {"ES256"};
    compare(*v, toks, ex3, kPaths, nullptr, "alg header", nullptr);
    // an Expected per token: each row is what its own Expected gives alone
    {
      Expected late = ex;
      late.now_unix_ns = (T0 + 7200) * 1000000000LL;          // every token has expired
      const std::vector<Expected> exs = {ex, late};
      std::vector<uint32_t> which(toks.size());
      for (size_t i = 0; i < which.size(); ++i) which[i] = (uint32_t)(i & 1);
      CheckStats s2;
      const auto rs = v->SelectBatchEach(toks, exs, which, kPaths, &s2);
      const auto r0 = v->SelectBatch(toks, exs[0], kPaths), r1 = v->SelectBatch(toks, exs[1], kPaths);
      for (size_t i = 0; i < rs.size(); ++i) {
        const SelectResult& w = which[i] ? r1[i] : r0[i];
        check(rs[i].ok == w.ok && rs[i].err == w.err && rs[i].values.size() == w.values.size(),
              "each: token " + std::to_string(i), rs[i].err + " / " + w.err);
        for (size_t k = 0; k < rs[i].values.size() && k < w.values.size(); ++k)
          check(show(rs[i].values[k]) == show(w.values[k]), "each: value", show(rs[i].values[k]));
      }
      check(s2.scanned == st.scanned && s2.host == st.host, "each: stats");
      check(rs[0].ok && !rs[1].ok && has(rs[1].err, "expired"), "each: the late profile rejects", rs[1].err);
    }
    // the columns hold the same rows; 120 copies of the batch, so that several merge threads write them
    for (const ClaimPaths& paths : {kPaths, refused[0]}) {
      std::vector<std::string_view> big;
      for (int rep = 0; rep < 120; ++rep) big.insert(big.end(), toks.begin(), toks.end());
      const auto rb = v->SelectBatch(big, ex, paths);
      const size_t n = big.size(), nn = paths.paths.size();
      std::vector<uint8_t> ok(n, 0xee), present(n, 0xee);
      std::vector<int64_t> dates[3] = {std::vector<int64_t>(n, -1), std::vector<int64_t>(n, -1), std::vector<int64_t>(n, -1)};
      std::vector<uint32_t> off[4];
      for (auto& o : off) o.assign(n + 1, 0xeeeeeeeeu);
      std::vector<char> var[5];
      SelectColumns S;
      RegisteredColumns& R = S.reg;
      R.ok = ok.data();
      R.present = present.data();
      R.exp = dates[0].data();
      R.nbf = dates[1].data();
      R.iat = dates[2].data();
      R.iss_off = off[0].data();
      R.sub_off = off[1].data();
      R.jti_off = off[2].data();
      R.aud_tok = off[3].data();
      R.alloc = [&](RegisteredColumns::Var which, size_t bytes) {
        var[which].assign(bytes, (char)0xee);
        return (void*)var[which].data();
      };
      std::vector<std::vector<uint8_t>> type(nn, std::vector<uint8_t>(n, 0xee));
      std::vector<std::vector<double>> num(nn, std::vector<double>(n, -7.0));
      std::vector<std::vector<uint32_t>> toff(nn, std::vector<uint32_t>(n + 1, 0xeeeeeeeeu));
      std::vector<std::vector<char>> text(nn);
      S.names.resize(nn);
      for (size_t k = 0; k < nn; ++k) {
        S.names[k].type = type[k].data();
        S.names[k].num = num[k].data();
        S.names[k].text_off = toff[k].data();
      }
      S.alloc_text = [&](size_t k, size_t bytes) {
        text[k].assign(bytes, (char)0xee);
        return (void*)text[k].data();
      };
      CheckStats cst;
      v->SelectCols(big, ex, paths, S, &cst);
      const bool scan = nn <= JG_MAX_PATHS;
      check(cst.scanned == (scan ? 120 * st.scanned : 0) && cst.host == (scan ? 120 * st.host : 120 * nc), "columns: stats");
      for (size_t k = 0; k < nn; ++k) check(toff[k][0] == 0 && toff[k][n] == text[k].size(), "columns: text size");
      for (size_t i = 0; i < n && !fails; ++i) {
        const std::string at = "columns: token " + std::to_string(i);
        check((ok[i] != 0) == rb[i].ok, at + " ok");
        for (size_t k = 0; k < nn; ++k) {
          const std::string cell(text[k].data() + toff[k][i], toff[k][i + 1] - toff[k][i]);
          const uint8_t t = type[k][i];
          const std::string nm = name_of(paths.paths[k]);
          if (!rb[i].ok || !rb[i].values[k]) {
            check(t == JG_SEL_ABSENT && cell.empty() && num[k][i] == 0.0, at + " " + nm + " absent");
            continue;
          }
          const json::Value& val = *rb[i].values[k];
          const bool host_row = !scan || cases[i % toks.size()].host;
          uint8_t want_t = val.kind == json::Value::Null     ? JG_SEL_NULL
                           : val.kind == json::Value::Bool   ? (val.b ? JG_SEL_TRUE : JG_SEL_FALSE)
                           : val.kind == json::Value::Number ? JG_SEL_NUMBER
                           : val.kind == json::Value::String ? JG_SEL_STRING
                           : val.kind == json::Value::Array  ? JG_SEL_ARRAY
                                                             : JG_SEL_OBJECT;
          if (!host_row && val.kind == json::Value::String)
            for (unsigned char ch : val.str.view())
              if (ch >= 0x80) want_t = JG_SEL_STRING_RAW;
          check(t == want_t, at + " " + nm + " type", std::to_string(t));
          const double want_num = val.kind == json::Value::Number ? val.num : 0.0;
          check(std::memcmp(&num[k][i], &want_num, 8) == 0, at + " " + nm + " num");
          const std::string want_text = val.kind == json::Value::String ? std::string(val.str.view())
                                        : (val.kind == json::Value::Array || val.kind == json::Value::Object)
                                            ? json::marshal(val) : std::string();
          check(cell == want_text, at + " " + nm + " text", cell);
        }
      }
    }
  } else if (mode == "nopaths") {
    const char* un = "capjwt: claims scan unavailable: capjwt: jg_claims_paths: not provided by the loaded verifier library";
    for (int round = 0; round < 2; ++round) {              // again after the context was recreated
      CheckStats st;
      const auto rs = v->SelectBatch(toks, ex, kPaths, &st);
      for (size_t i = 0; i < toks.size(); ++i) {
        if (i == nc) check(!rs[i].ok && !has(rs[i].err, "unavailable"), "nopaths: parse error", rs[i].err);
        else check(!rs[i].ok && rs[i].err == un && rs[i].values.empty(), "nopaths: token " + std::to_string(i), rs[i].err);
      }
      check(st.scanned == 0 && st.host == 0, "nopaths: stats");
    }
    const auto gs = v->SelectBatch(toks, ex, {"scope", "cnf"});          // the scan by name is there
    check(gs[0].ok && show(gs[0].values[0]) == "\"r w\"" && !gs[5].ok, "nopaths: SelectBatch by name works", gs[0].err);
    // a refused path list never reaches the scan: the host path answers
    const auto hs = v->SelectBatch(toks, ex, ClaimPaths{{{"cnf", "jkt"}, {"cnf", ""}}});
    check(hs[0].ok && show(hs[0].values[0]) == "\"0Zc\"", "nopaths: host path", hs[0].err);
  } else {
    std::printf("unknown mode %s\n", mode.c_str());
    return 2;
  }
  std::printf(fails ? "paths %s: %d failures\n" : "paths %s: ok\n", mode.c_str(), fails);
  return fails ? 1 : 0;
}
