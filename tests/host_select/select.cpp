// select.cpp -- Validator::SelectBatch's host merge without a GPU.
//
//   select ok        linked with select_stub.cpp: the values of device-decided
//                    rows (from the scan's jg_selected records) and of JG_CL_HOST
//                    rows (from the verified claims map) equal ValidateBatch's map
//                    entries and the JSON written below; ok / err are CheckBatch's
//                    and the claims RegisteredBatch's, token for token; a name
//                    list the ABI refuses takes the host path for every token;
//                    SelectCols holds the same rows
//   select noselect  linked with select_stub.cpp built -DNO_SELECT: every token
//                    that reaches the scan gets "claims scan unavailable",
//                    RegisteredBatch still works
//   select fault     linked with tests/host_faults/fault_stub.cpp (no select
//                    symbol, every device call fails): per-token errors, no crash
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

struct Case {
  std::string payload;
  bool ok;
  bool host;                                   // the scan leaves it to the host
  std::vector<std::string> want;               // json::marshal of the value per name of kNames, or kAbsent
};

static const std::vector<std::string> kNames = {"scope", "roles", "n", "t", "missing"};

// the rows of one SelectBatch against ValidateBatch / CheckBatch / RegisteredBatch and the cases' JSON
static void compare(Validator& v, const std::vector<std::string_view>& toks, const Expected& ex,
                    const std::vector<std::string>& names, const std::vector<Case>* cases, const std::string& tag,
                    CheckStats* st) {
  const auto rs = v.SelectBatch(toks, ex, names, st);
  const auto cs = v.CheckBatch(toks, ex);
  const auto gs = v.RegisteredBatch(toks, ex);
  Results vs = v.ValidateBatch(toks, ex);
  check(rs.size() == toks.size(), tag + " size");
  for (size_t i = 0; i < rs.size(); ++i) {
    const std::string at = tag + " token " + std::to_string(i);
    check(rs[i].ok == cs[i].ok && rs[i].err == cs[i].err, at + " differs from CheckBatch", rs[i].err + " / " + cs[i].err);
    check(rs[i].ok == vs[i].ok && rs[i].err == vs[i].err, at + " differs from ValidateBatch", rs[i].err + " / " + vs[i].err);
    const RegisteredClaims &a = rs[i].claims, &b = gs[i].claims;
    check(a.Issuer == b.Issuer && a.Subject == b.Subject && a.ID == b.ID && a.Audience == b.Audience &&
              a.Expiry == b.Expiry && a.NotBefore == b.NotBefore && a.IssuedAt == b.IssuedAt,
          at + " claims differ from RegisteredBatch");
    if (!rs[i].ok) {
      check(rs[i].values.empty(), at + ": a rejected token carries values");
      continue;
    }
    check(rs[i].values.size() == names.size(), at + " values size");
    for (size_t k = 0; k < names.size() && k < rs[i].values.size(); ++k) {
      const std::string got = show(rs[i].values[k]);
      check(got == show(vs[i].claims.get(names[k])), at + " " + names[k] + " differs from ValidateBatch's map",
            got + " / " + show(vs[i].claims.get(names[k])));
      const json::Value* m = vs[i].claims.get(names[k]);
      if (m && rs[i].values[k])
        check(m->kind == rs[i].values[k]->kind && std::memcmp(&m->num, &rs[i].values[k]->num, 8) == 0,
              at + " " + names[k] + " kind / float bits");
      if (cases && i < cases->size() && &names == &kNames) check(got == (*cases)[i].want[k], at + " " + names[k], got);
    }
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "ok";
  const int64_t T0 = 1611699344;
  const std::string A = kAbsent;
  const std::vector<Case> cases = {
      // decided by the scan: the values come from the records
      {R"({"scope":"read write","roles":["admin","dev"],"n":1.5,"t":true,"exp":1611699944})", true, false,
       {"\"read write\"", "[\"admin\",\"dev\"]", "1.5", "true", A}},
      {R"({"exp":1611699944,"roles":[ 1 , "a" ,	{ "k" : [ ] } ],"scope":"","n":-0,"t":null})", true, false,
       {"\"\"", "[1,\"a\",{\"k\":[]}]", "-0", "null", A}},
      {R"({"exp":1611699944,"scope":{"b":1,"a":[true,false]},"n":12345678901234567,"t":false,"Scope":"x"})", true, false,
       {"{\"a\":[true,false],\"b\":1}", A, "12345678901234568", "false", A}},   // the float64 nearest to the literal
      {R"({"scope":"first","x":{"scope":"inner","roles":1},"scope":[2],"exp":1611699944,"n":0})", true, false,
       {"[2]", A, "0", A, A}},
      {"{\"scope\":\"J\xc3\xbcrgen\",\"roles\":\"a\xff" "b\",\"exp\":1611699944}", true, false,
       {"\"J\xc3\xbcrgen\"", "\"a\xef\xbf\xbd" "b\"", A, A, A}},
      {R"({"exp":1611699944})", true, false, {A, A, A, A, A}},
      {R"({"exp":1611698344,"scope":"late"})", false, false, {}},
      // left to the host: the values come from the verified claims map
      {R"({"scope":"a\/b","roles":[ 1 , "a" ,	{ "k" : [ ] } ],"n":1e3,"t":true,"exp":1611699944})", true, true,
       {"\"a/b\"", "[1,\"a\",{\"k\":[]}]", "1000", "true", A}},
      {R"({"exp":1611699944,"EXP":1611699945,"scope":null,"roles":{"z":1,"a":2}})", true, true,
       {"null", "{\"a\":2,\"z\":1}", A, A, A}},
      {R"({"sub":5,"exp":1611699944,"scope":"x"})", false, true, {}},
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
    compare(*v, toks, ex, kNames, &cases, "five names", &st);
    for (size_t i = 0; i < nc; ++i) {
      const auto one = v->SelectBatch({toks[i]}, ex, kNames);
      check(one[0].ok == cases[i].ok, "case " + std::to_string(i) + " verdict", one[0].err);
    }
    check(st.host == want_host && st.scanned == nc - want_host, "stats",
          std::to_string(st.scanned) + " scanned, " + std::to_string(st.host) + " host");
    // no names, one name, eight names: still the scan
    for (const std::vector<std::string>& names :
         {std::vector<std::string>{}, std::vector<std::string>{"roles"},
          std::vector<std::string>{"a", "b", "c", "d", "scope", "roles", "n", "t"}}) {
      CheckStats s2;
      compare(*v, toks, ex, names, nullptr, std::to_string(names.size()) + " names", &s2);
      check(s2.scanned == st.scanned && s2.host == st.host, std::to_string(names.size()) + " names: stats");
    }
    // equal names share a slot: eight distinct names and a repeat is still the scan
    {
      const std::vector<std::string> names = {"scope", "a", "b", "c", "d", "roles", "n", "scope", "t", "roles"};
      CheckStats s2;
      compare(*v, toks, ex, names, nullptr, "repeated names", &s2);
      check(s2.scanned == st.scanned, "repeated names: stats");
    }
    // a name list the ABI refuses: every token takes the host path, the values are the same
    const std::vector<std::vector<std::string>> refused = {
        {"scope", "roles", "n", "t", "a", "b", "c", "d", "e"},        // nine names
        {"scope", std::string(65, 'L')},                             // a name over 64 bytes
        {"scope", "r\xc3\xb4les"},                                    // non-ASCII bytes
        {"scope", "ro\"les"}, {"scope", "ro\\les"}, {"scope", ""},   // a quote, a backslash, an empty name
    };
    for (size_t r = 0; r < refused.size(); ++r) {
      CheckStats s2;
      compare(*v, toks, ex, refused[r], nullptr, "refused list " + std::to_string(r), &s2);
      check(s2.scanned == 0 && s2.host == nc, "refused list " + std::to_string(r) + ": stats",
            std::to_string(s2.scanned) + " scanned, " + std::to_string(s2.host) + " host");
    }
    {
      const auto rs = v->SelectBatch(toks, ex, refused[0]);
      check(rs[0].ok && show(rs[0].values[1]) == "[\"admin\",\"dev\"]", "nine names: values", show(rs[0].values[1]));
    }
    bool threw = false;
    try {
      v->SelectBatch(toks, ex, {"scope", std::string("a\0b", 3)});
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    check(threw, "a name with a NUL byte is refused with an exception");
    check(v->SelectBatch({}, ex, kNames).empty(), "empty batch");
    // the alg header check stays on the host and comes ahead of any claim error
    Expected ex3 = ex;
    ex3.SigningAlgorithms = {"ES256"};
    compare(*v, toks, ex3, kNames, nullptr, "alg header", nullptr);
    // the columns hold the same rows; 120 copies of the batch, so that several merge threads write them
    for (const std::vector<std::string>& names : {kNames, refused[0]}) {
      std::vector<std::string_view> big;
      for (int rep = 0; rep < 120; ++rep) big.insert(big.end(), toks.begin(), toks.end());
      const auto rb = v->SelectBatch(big, ex, names);
      const size_t n = big.size(), nn = names.size();
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
      v->SelectCols(big, ex, names, S, &cst);
      const bool scan = names.size() <= JG_MAX_SELECT;
      check(cst.scanned == (scan ? 120 * st.scanned : 0) && cst.host == (scan ? 120 * st.host : 120 * nc), "columns: stats");
      for (size_t k = 0; k < nn; ++k) check(toff[k][0] == 0 && toff[k][n] == text[k].size(), "columns: text size");
      for (size_t i = 0; i < n && !fails; ++i) {
        const std::string at = "columns: token " + std::to_string(i);
        check((ok[i] != 0) == rb[i].ok, at + " ok");
        check(std::string(var[1].data() + off[1][i], off[1][i + 1] - off[1][i]) == rb[i].claims.Subject, at + " sub");
        for (size_t k = 0; k < nn; ++k) {
          const std::string cell(text[k].data() + toff[k][i], toff[k][i + 1] - toff[k][i]);
          const uint8_t t = type[k][i];
          if (!rb[i].ok || !rb[i].values[k]) {
            check(t == JG_SEL_ABSENT && cell.empty() && num[k][i] == 0.0, at + " " + names[k] + " absent");
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
          check(t == want_t, at + " " + names[k] + " type", std::to_string(t));
          const double want_num = val.kind == json::Value::Number ? val.num : 0.0;
          check(std::memcmp(&num[k][i], &want_num, 8) == 0, at + " " + names[k] + " num");
          const std::string want_text = val.kind == json::Value::String ? std::string(val.str.view())
                                        : (val.kind == json::Value::Array || val.kind == json::Value::Object)
                                            ? json::marshal(val) : std::string();
          check(cell == want_text, at + " " + names[k] + " text", cell);
        }
      }
      // an array's text is json::marshal's on both paths: the same bytes from a record and from the map
      if (scan) {
        const std::string dev(text[1].data() + toff[1][1], toff[1][2] - toff[1][1]);
        const std::string hst(text[1].data() + toff[1][7], toff[1][8] - toff[1][7]);
        check(dev == "[1,\"a\",{\"k\":[]}]" && dev == hst && !cases[1].host && cases[7].host, "columns: array text", dev + " / " + hst);
      }
    }
  } else if (mode == "noselect") {
    const char* un = "capjwt: claims scan unavailable: capjwt: jg_claims_select: not provided by the loaded verifier library";
    for (int round = 0; round < 2; ++round) {              // again after the context was recreated
      CheckStats st;
      const auto rs = v->SelectBatch(toks, ex, kNames, &st);
      for (size_t i = 0; i < toks.size(); ++i) {
        if (i == nc) check(!rs[i].ok && !has(rs[i].err, "unavailable"), "noselect: parse error", rs[i].err);
        else check(!rs[i].ok && rs[i].err == un && rs[i].values.empty(), "noselect: token " + std::to_string(i), rs[i].err);
      }
      check(st.scanned == 0 && st.host == 0, "noselect: stats");
    }
    const auto gs = v->RegisteredBatch(toks, ex);          // the scan with records alone is there
    check(gs[0].ok && !gs[6].ok, "noselect: RegisteredBatch works", gs[0].err);
    // a refused name list never reaches the scan: the host path answers
    const auto hs = v->SelectBatch(toks, ex, {"scope", ""});
    check(hs[0].ok && show(hs[0].values[0]) == "\"read write\"", "noselect: host path", hs[0].err);
  } else if (mode == "fault") {
    const auto rs = v->SelectBatch(toks, ex, kNames);
    check(rs.size() == toks.size(), "fault: size");
    for (size_t i = 0; i < rs.size(); ++i) {
      if (i == nc) check(!rs[i].ok && !has(rs[i].err, "unavailable"), "fault: parse error", rs[i].err);
      else check(!rs[i].ok && has(rs[i].err, "unavailable: "), "fault: token " + std::to_string(i), rs[i].err);
      check(rs[i].values.empty() && rs[i].claims.Subject.empty(), "fault: no values");
    }
  } else {
    std::printf("unknown mode %s\n", mode.c_str());
    return 2;
  }
  std::printf(fails ? "select %s: %d failures\n" : "select %s: ok\n", mode.c_str(), fails);
  return fails ? 1 : 0;
}
