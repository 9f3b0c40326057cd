// registered.cpp -- Validator::RegisteredBatch's host merge without a GPU.
//
//   registered ok         linked with accept_stub.cpp: the claims of plain
//                         payloads (from the scan's records) and of hard ones
//                         (JG_CL_HOST: from the struct validate_claims decodes)
//                         equal the values written below; ok / err are
//                         CheckBatch's, token for token
//   registered noextract  linked with accept_stub.cpp built -DNO_EXTRACT: every
//                         token that reaches the scan gets "claims scan
//                         unavailable", CheckBatch still works
//   registered fault      linked with tests/host_faults/fault_stub.cpp (no
//                         extract symbol, every device call fails): per-token
//                         errors, no crash
// Prints FAIL lines and exits 1 on a mismatch.
#include <cstdio>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/host/cap_jwt.hpp"

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

using Date = std::optional<int64_t>;
struct Case {
  std::string payload;
  bool ok;
  std::string err;
  bool host;                                   // the scan leaves it to the host
  std::string iss, sub, jti;
  std::vector<std::string> aud;
  Date exp, nbf, iat;
};

static std::string show(const RegisteredClaims& c) {
  auto d = [](const Date& x) { return x ? std::to_string(*x) : std::string("nil"); };
  std::string s = "iss=" + c.Issuer + " sub=" + c.Subject + " jti=" + c.ID + " aud=[";
  for (const auto& a : c.Audience) s += a + "|";
  return s + "] exp=" + d(c.Expiry) + " nbf=" + d(c.NotBefore) + " iat=" + d(c.IssuedAt);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "ok";
  const int64_t T0 = 1611699344;
  const Date none;
  const std::vector<Case> cases = {
      // decided by the scan: the claims come from the records
      {R"({"iss":"https://example.com/","sub":"alice","aud":["a","b"],"exp":1611699944,"iat":1611699344,"jti":"id1"})",
       true, "", false, "https://example.com/", "alice", "id1", {"a", "b"}, 1611699944, none, 1611699344},
      {R"({"aud":"solo","nbf":1611699339,"sub":""})", true, "", false, "", "", "", {"solo"}, none, 1611699339, none},
      {R"({"exp":null,"iat":1611699344,"aud":[],"jti":null,"x":{"sub":"inner"}})", true, "", false, "", "", "", {}, none,
       none, 1611699344},
      {R"({"pad":"x","sub":"a","exp":1611699944})", true, "", false, "", "a", "", {}, 1611699944, none, none},
      {R"({"pad":"xx","sub":"ab","exp":1611699944})", true, "", false, "", "ab", "", {}, 1611699944, none, none},
      {R"({ "aud" : [ "one" ,	"two", "" ] , "exp":0, "nbf":1611699344 })", true, "", false, "", "", "",
       {"one", "two", ""}, 0, 1611699344, none},
      {R"({"exp":1611698344,"sub":"late"})", false, "invalid expiration time (exp) claim: token is expired", false, "",
       "", "", {}, none, none, none},
      {R"({"sub":"timeless"})", false, "no issued at (iat), not before (nbf), or expiration time (exp) claims in token",
       false, "", "", "", {}, none, none, none},
      // left to the host: the claims come from the struct validate_claims decodes
      {R"({"sub":"alice","exp":1611699944,"aud":"x\/y"})", true, "", true, "", "alice", "", {"x/y"}, 1611699944,
       none, none},
      {"{\"iss\":\"\xc3\xa9\",\"aud\":[\"\xc3\xa9\",\"b\"],\"exp\":1611699944.5,\"iat\":null}", true, "", true,
       "\xc3\xa9", "", "", {"\xc3\xa9", "b"}, 1611699944, none, none},
      // named twice: Go assigns in sorted key order, "EXP" before "exp"
      {R"({"exp":1611699944,"EXP":1611699945,"jti":"dup"})", true, "", true, "", "", "dup", {}, 1611699944, none, none},
      {R"({"sub":5,"exp":1611699944})", false, "json: cannot unmarshal into Go struct field Claims.sub of type string",
       true, "", "", "", {}, none, none, none},
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
    CheckStats st, cst;
    const auto rs = v->RegisteredBatch(toks, ex, &st);
    const auto cs = v->CheckBatch(toks, ex, &cst);
    check(rs.size() == toks.size() && cs.size() == toks.size(), "sizes");
    size_t want_host = 0;
    for (size_t i = 0; i < toks.size(); ++i) {
      check(rs[i].ok == cs[i].ok && rs[i].err == cs[i].err, "token " + std::to_string(i) + " differs from CheckBatch",
            rs[i].err + " / " + cs[i].err);
      if (!rs[i].ok) {
        const RegisteredClaims& c = rs[i].claims;
        check(c.Issuer.empty() && c.Subject.empty() && c.ID.empty() && c.Audience.empty() && !c.Expiry &&
                  !c.NotBefore && !c.IssuedAt,
              "token " + std::to_string(i) + ": a rejected token carries claims", show(c));
      }
    }
    for (size_t i = 0; i < nc; ++i) {
      const Case& c = cases[i];
      want_host += c.host;
      const std::string tag = "case " + std::to_string(i);
      check(rs[i].ok == c.ok && rs[i].err == c.err, tag + " verdict", rs[i].err);
      if (!c.ok) continue;
      const RegisteredClaims& g = rs[i].claims;
      check(g.Issuer == c.iss && g.Subject == c.sub && g.ID == c.jti && g.Audience == c.aud && g.Expiry == c.exp &&
                g.NotBefore == c.nbf && g.IssuedAt == c.iat,
            tag + " claims", show(g));
    }
    check(!rs[nc].ok && !rs[nc].err.empty() && has(rs[nc].err, "error verifying token signature: "), "parse error",
          rs[nc].err);
    check(st.host == want_host && st.scanned == nc - want_host, "stats",
          std::to_string(st.scanned) + " scanned, " + std::to_string(st.host) + " host");
    check(st.scanned == cst.scanned && st.host == cst.host, "stats equal CheckBatch's");
    // a claim check that fails on a device-decided and on a host-decided token
    Expected ex2 = ex;
    ex2.Subject = "alice";
    const auto r2 = v->RegisteredBatch(toks, ex2);
    const auto c2 = v->CheckBatch(toks, ex2);
    for (size_t i = 0; i < toks.size(); ++i)
      check(r2[i].ok == c2[i].ok && r2[i].err == c2[i].err, "subject: token " + std::to_string(i), r2[i].err);
    check(r2[0].ok && r2[0].claims.Subject == "alice" && r2[8].ok && r2[8].claims.Subject == "alice", "subject: accepted");
    check(!r2[1].ok && r2[1].err == "invalid subject (sub) claim" && !r2[10].ok && r2[10].err == r2[1].err,
          "subject: rejected", r2[1].err + " / " + r2[10].err);
    // the alg header check stays on the host and comes ahead of any claim error
    Expected ex3 = ex;
    ex3.SigningAlgorithms = {"ES256"};
    const auto r3 = v->RegisteredBatch(toks, ex3);
    const auto c3 = v->CheckBatch(toks, ex3);
    for (size_t i = 0; i < nc; ++i)
      check(!r3[i].ok && r3[i].err == c3[i].err && r3[i].claims.Subject.empty() &&
                r3[i].err == "invalid algorithm (alg) header parameter: token signed with unexpected algorithm",
            "alg header: token " + std::to_string(i), r3[i].err);
    check(v->RegisteredBatch({}, ex).empty(), "empty batch");
    // the columns hold the same rows; 120 copies of the batch, so that several merge threads write them
    {
      std::vector<std::string_view> big;
      for (int rep = 0; rep < 120; ++rep) big.insert(big.end(), toks.begin(), toks.end());
      const auto rb = v->RegisteredBatch(big, ex);
      const size_t n = big.size();
      std::vector<uint8_t> ok(n, 0xee), present(n, 0xee);
      std::vector<int64_t> dates[3] = {std::vector<int64_t>(n, -1), std::vector<int64_t>(n, -1), std::vector<int64_t>(n, -1)};
      std::vector<uint32_t> off[4];
      for (auto& o : off) o.assign(n + 1, 0xeeeeeeeeu);
      std::vector<char> var[5];
      RegisteredColumns R;
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
      CheckStats cst2;
      v->RegisteredCols(big, ex, R, &cst2);
      check(cst2.scanned == 120 * st.scanned && cst2.host == 120 * st.host, "columns: stats");
      const uint32_t* aud_off = (const uint32_t*)var[RegisteredColumns::AUD_OFF].data();
      check(var[RegisteredColumns::AUD_OFF].size() == 4 * ((size_t)off[3][n] + 1) && aud_off[0] == 0 &&
                aud_off[off[3][n]] == var[RegisteredColumns::AUD].size() && off[0][0] == 0 &&
                off[0][n] == var[RegisteredColumns::ISS].size() && off[1][n] == var[RegisteredColumns::SUB].size() &&
                off[2][n] == var[RegisteredColumns::JTI].size(),
            "columns: sizes");
      for (size_t i = 0; i < n && !fails; ++i) {
        const RegisteredClaims& g = rb[i].claims;
        auto cut = [&](int which, const uint32_t* o, size_t k) {
          return std::string(var[which].data() + o[k], o[k + 1] - o[k]);
        };
        std::vector<std::string> aud;
        for (uint32_t k = off[3][i]; k < off[3][i + 1]; ++k) aud.push_back(cut(RegisteredColumns::AUD, aud_off, k));
        auto date = [&](int k) { return (present[i] >> (5 + k)) & 1 ? Date(dates[k][i]) : Date(); };
        check((ok[i] != 0) == rb[i].ok && (present[i] & 0x1f) == 0 && cut(0, off[0].data(), i) == g.Issuer &&
                  cut(1, off[1].data(), i) == g.Subject && cut(2, off[2].data(), i) == g.ID && aud == g.Audience &&
                  date(0) == g.Expiry && date(1) == g.NotBefore && date(2) == g.IssuedAt &&
                  dates[0][i] == g.Expiry.value_or(0) && dates[1][i] == g.NotBefore.value_or(0) &&
                  dates[2][i] == g.IssuedAt.value_or(0),
              "columns: token " + std::to_string(i), show(g));
      }
      uint32_t one[4] = {7, 7, 7, 7};
      RegisteredColumns Z = R;
      Z.iss_off = &one[0];
      Z.sub_off = &one[1];
      Z.jti_off = &one[2];
      Z.aud_tok = &one[3];
      v->RegisteredCols({}, ex, Z);
      check(one[0] == 0 && one[3] == 0 && var[RegisteredColumns::AUD_OFF].size() == 4 && var[0].empty(),
            "columns: empty batch");
    }
  } else if (mode == "noextract") {
    const char* un = "capjwt: claims scan unavailable: capjwt: jg_claims_extract: not provided by the loaded verifier library";
    for (int round = 0; round < 2; ++round) {              // again after the context was recreated
      CheckStats st;
      const auto rs = v->RegisteredBatch(toks, ex, &st);
      for (size_t i = 0; i < toks.size(); ++i) {
        if (i == nc) check(!rs[i].ok && !has(rs[i].err, "unavailable"), "noextract: parse error", rs[i].err);
        else check(!rs[i].ok && rs[i].err == un, "noextract: token " + std::to_string(i), rs[i].err);
      }
      check(st.scanned == 0 && st.host == 0, "noextract: stats");
    }
    const auto cs = v->CheckBatch(toks, ex);                // the scan without records is there
    check(cs[0].ok && !cs[6].ok && cs[6].err == cases[6].err, "noextract: CheckBatch works", cs[0].err);
  } else if (mode == "fault") {
    const auto rs = v->RegisteredBatch(toks, ex);
    check(rs.size() == toks.size(), "fault: size");
    for (size_t i = 0; i < rs.size(); ++i) {
      if (i == nc) check(!rs[i].ok && !has(rs[i].err, "unavailable"), "fault: parse error", rs[i].err);
      else check(!rs[i].ok && has(rs[i].err, "unavailable: "), "fault: token " + std::to_string(i), rs[i].err);
      check(rs[i].claims.Subject.empty() && rs[i].claims.Audience.empty(), "fault: no claims");
    }
  } else {
    std::printf("unknown mode %s\n", mode.c_str());
    return 2;
  }
  std::printf(fails ? "registered %s: %d failures\n" : "registered %s: ok\n", mode.c_str(), fails);
  return fails ? 1 : 0;
}
