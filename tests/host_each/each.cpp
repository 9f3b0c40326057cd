// each.cpp -- the Validator::*Each entries (an Expected per token) without a GPU.
//
//   each ok      linked with each_stub.cpp: for a batch of three tenants whose
//                profiles differ in issuer, audiences, Now and SigningAlgorithms
//                -- with wrong-tenant tokens, tokens expired for one profile only,
//                payloads the scan leaves to the host, a profile with 17
//                audiences (no device slot) and a batch with 65 profiles in use --
//                CheckBatchEach, CheckVerdictsEach, RegisteredBatchEach,
//                RegisteredColsEach, SelectBatchEach and SelectColsEach equal the
//                existing entry called once per profile group and scattered back;
//                the stats sum up; one scan call per batch; the three
//                std::invalid_argument cases
//   each noeach  linked with each_stub.cpp built -DNO_EACH: every token that
//                reaches the scan gets "claims scan unavailable", tokens of the
//                profile without a slot still take the host path, and the
//                existing entries still work
// Prints FAIL lines and exits 1 on a mismatch.
#include <cstdio>
#include <cstring>
#include <functional>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../cap_amd/csrc/host/cap_jwt.hpp"
#include "../../include/jg.h"

using namespace capjwt;

extern "C" int each_stub_calls;
extern "C" int each_stub_profiles;

static int fails = 0;
static void check(bool ok, const std::string& what, const std::string& got = "") {
  if (!ok) {
    std::printf("FAIL %s: %s\n", what.c_str(), got.c_str());
    ++fails;
  }
}
static bool has(const std::string& s, const char* sub) { return s.find(sub) != std::string::npos; }

static std::string token(const std::string& payload, const char* alg = "EdDSA") {
  return b64url_encode(std::string(R"({"alg":")") + alg + R"(","kid":"k1"})") + "." + b64url_encode(payload) + "." +
         std::string(86, 'A');
}
static std::string show(const std::optional<json::Value>& v) { return v ? json::marshal(*v) : std::string("<absent>"); }
static bool same_claims(const RegisteredClaims& a, const RegisteredClaims& b) {
  return a.Issuer == b.Issuer && a.Subject == b.Subject && a.ID == b.ID && a.Audience == b.Audience &&
         a.Expiry == b.Expiry && a.NotBefore == b.NotBefore && a.IssuedAt == b.IssuedAt;
}

static const int64_t T0 = 1611699344;
static const std::vector<std::string> kNames = {"scope", "roles", "n", "missing"};

struct Batch {
  std::vector<std::string> store;
  std::vector<uint32_t> which;
  std::vector<std::string_view> toks() const { return {store.begin(), store.end()}; }
  void add(uint32_t p, const std::string& payload, const char* alg = "EdDSA") {
    store.push_back(token(payload, alg));
    which.push_back(p);
  }
};

// the tokens of profile p and where they sit
static std::vector<size_t> group(const Batch& b, uint32_t p) {
  std::vector<size_t> at;
  for (size_t i = 0; i < b.which.size(); ++i)
    if (b.which[i] == p) at.push_back(i);
  return at;
}

// what the *Cols entries write, kept by value
struct Cols {
  size_t n, nn;
  std::vector<uint8_t> ok, present;
  std::vector<int64_t> exp;
  std::vector<int64_t> nbf, iat;
  std::vector<uint32_t> off[4];
  std::vector<char> var[5];
  std::vector<std::vector<uint8_t>> type;
  std::vector<std::vector<double>> num;
  std::vector<std::vector<uint32_t>> toff;
  std::vector<std::vector<char>> text;
  SelectColumns S;
  Cols(size_t n_, size_t nn_)
      : n(n_), nn(nn_), ok(n_, 0xee), present(n_, 0xee), exp(n_, -1), nbf(n_, -1), iat(n_, -1),
        type(nn_, std::vector<uint8_t>(n_, 0xee)), num(nn_, std::vector<double>(n_, -7.0)),
        toff(nn_, std::vector<uint32_t>(n_ + 1, 0xeeeeeeeeu)), text(nn_) {
    for (auto& o : off) o.assign(n + 1, 0xeeeeeeeeu);
    RegisteredColumns& R = S.reg;
    R.ok = ok.data();
    R.present = present.data();
    R.exp = exp.data();
    R.nbf = nbf.data();
    R.iat = iat.data();
    R.iss_off = off[0].data();
    R.sub_off = off[1].data();
    R.jti_off = off[2].data();
    R.aud_tok = off[3].data();
    R.alloc = [this](RegisteredColumns::Var w, size_t bytes) {
      var[w].assign(bytes, (char)0xee);
      return (void*)var[w].data();
    };
    S.names.resize(nn);
    for (size_t k = 0; k < nn; ++k) {
      S.names[k].type = type[k].data();
      S.names[k].num = num[k].data();
      S.names[k].text_off = toff[k].data();
    }
    S.alloc_text = [this](size_t k, size_t bytes) {
      text[k].assign(bytes, (char)0xee);
      return (void*)text[k].data();
    };
  }
  std::string str(int w, size_t i) const { return std::string(var[w].data() + off[w][i], off[w][i + 1] - off[w][i]); }
  std::string cell(size_t k, size_t i) const { return std::string(text[k].data() + toff[k][i], toff[k][i + 1] - toff[k][i]); }
};

// every *Each entry on (b, exps) against the existing entry per profile group; *sum: the groups' stats
static void compare(Validator& v, const Batch& b, const std::vector<Expected>& exps, const std::string& tag,
                    CheckStats* each_stats, CheckStats* sum) {
  const auto toks = b.toks();
  const size_t n = toks.size();
  std::vector<CheckResult> want_c(n);
  std::vector<RegisteredResult> want_r(n);
  std::vector<SelectResult> want_s(n);
  Results want_v(n);
  *sum = CheckStats{};
  for (uint32_t p = 0; p < exps.size(); ++p) {
    const auto at = group(b, p);
    if (at.empty()) continue;
    std::vector<std::string_view> part;
    for (size_t i : at) part.push_back(toks[i]);
    CheckStats st;
    auto c = v.CheckBatch(part, exps[p], &st);
    auto r = v.RegisteredBatch(part, exps[p]);
    auto s = v.SelectBatch(part, exps[p], kNames);
    auto val = v.ValidateBatch(part, exps[p]);
    sum->scanned += st.scanned;
    sum->host += st.host;
    for (size_t k = 0; k < at.size(); ++k) {
      want_c[at[k]] = std::move(c[k]);
      want_r[at[k]] = std::move(r[k]);
      want_s[at[k]] = std::move(s[k]);
      want_v[at[k]] = std::move(val[k]);
    }
  }
  const int calls0 = each_stub_calls;
  CheckStats sc, sr, ss, sv, srcol, sscol;
  const auto c = v.CheckBatchEach(toks, exps, b.which, &sc);
  check(each_stub_calls == calls0 + 1, tag + ": one scan call for the batch", std::to_string(each_stub_calls - calls0));
  const auto bits = v.CheckVerdictsEach(toks, exps, b.which, &sv);
  const auto r = v.RegisteredBatchEach(toks, exps, b.which, &sr);
  const auto s = v.SelectBatchEach(toks, exps, b.which, kNames, &ss);
  check(each_stub_calls == calls0 + 4, tag + ": one scan call per entry");
  Cols rc(n, 0), qc(n, kNames.size());
  v.RegisteredColsEach(toks, exps, b.which, rc.S.reg, &srcol);
  v.SelectColsEach(toks, exps, b.which, kNames, qc.S, &sscol);
  check(c.size() == n && bits.size() == n && r.size() == n && s.size() == n, tag + " sizes");
  for (const CheckStats* st : {&sv, &sr, &ss, &srcol, &sscol})
    check(st->scanned == sc.scanned && st->host == sc.host, tag + ": the entries' stats agree");
  *each_stats = sc;
  size_t accepted = 0;
  for (size_t i = 0; i < n && fails < 20; ++i) {
    const std::string at = tag + " token " + std::to_string(i) + " (profile " + std::to_string(b.which[i]) + ")";
    check(c[i].ok == want_c[i].ok && c[i].err == want_c[i].err, at + " CheckBatchEach", c[i].err + " / " + want_c[i].err);
    check(c[i].ok == want_v[i].ok && c[i].err == want_v[i].err, at + " against ValidateBatch", c[i].err + " / " + want_v[i].err);
    check((bits[i] != 0) == want_c[i].ok, at + " CheckVerdictsEach");
    check(r[i].ok == want_r[i].ok && r[i].err == want_r[i].err && same_claims(r[i].claims, want_r[i].claims),
          at + " RegisteredBatchEach", r[i].err + " / " + want_r[i].err);
    check(s[i].ok == want_s[i].ok && s[i].err == want_s[i].err && same_claims(s[i].claims, want_s[i].claims),
          at + " SelectBatchEach", s[i].err + " / " + want_s[i].err);
    check(s[i].values.size() == want_s[i].values.size(), at + " values size");
    for (size_t k = 0; k < s[i].values.size() && k < want_s[i].values.size(); ++k)
      check(show(s[i].values[k]) == show(want_s[i].values[k]), at + " " + kNames[k],
            show(s[i].values[k]) + " / " + show(want_s[i].values[k]));
    // the columns hold the rows
    for (const Cols* C : {&rc, &qc}) {
      check((C->ok[i] != 0) == r[i].ok, at + " columns ok");
      check(C->str(0, i) == r[i].claims.Issuer && C->str(1, i) == r[i].claims.Subject && C->str(2, i) == r[i].claims.ID,
            at + " columns strings", C->str(0, i));
      check(C->exp[i] == (r[i].claims.Expiry ? *r[i].claims.Expiry : 0), at + " columns exp");
      check(C->off[3][i + 1] - C->off[3][i] == r[i].claims.Audience.size(), at + " columns aud count");
    }
    for (size_t k = 0; k < kNames.size(); ++k) {
      const bool there = s[i].ok && s[i].values[k];
      check((qc.type[k][i] != JG_SEL_ABSENT) == there, at + " column type of " + kNames[k]);
      if (there && s[i].values[k]->kind == json::Value::String)
        check(qc.cell(k, i) == std::string(s[i].values[k]->str.view()), at + " column text of " + kNames[k]);
      if (there && s[i].values[k]->kind == json::Value::Array)
        check(qc.cell(k, i) == json::marshal(*s[i].values[k]), at + " column text of " + kNames[k]);
      if (there && s[i].values[k]->kind == json::Value::Number)
        check(qc.num[k][i] == s[i].values[k]->num, at + " column num of " + kNames[k]);
    }
    accepted += c[i].ok;
  }
  check(accepted > 0 && accepted < n, tag + ": some accepted, some rejected", std::to_string(accepted));
}

template <class F>
static bool throws_invalid(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "ok";
  PublicKey ed;
  ed.kind = PublicKey::Ed25519;
  ed.x = std::string(32, '\0');
  std::string err;
  auto ks = NewStaticKeySet({ed}, &err);
  check(ks != nullptr, "static key set", err);
  if (!ks) return 1;
  auto v = NewValidator(ks.get(), &err);

  // three tenants, a profile that takes ES256 alone, and one with 17 audiences
  auto profile = [&](const std::string& iss, std::vector<std::string> aud, int64_t now_s,
                     std::vector<std::string> algs) {
    Expected e;
    e.Issuer = iss;
    e.Audiences = std::move(aud);
    e.SigningAlgorithms = std::move(algs);
    e.has_now = true;
    e.now_unix_ns = now_s * 1000000000LL;
    e.NotBeforeLeeway = 3600 * 1000000000LL;      // a token with exp alone: nbf defaults to an hour before it
    return e;
  };
  std::vector<Expected> exps = {
      profile("https://a.example/", {"client-a"}, T0, {"EdDSA"}),
      profile("https://b.example/", {"client-b", "client-b2"}, T0, {"ES256", "EdDSA"}),
      profile("https://c.example/", {"client-c"}, T0 + 1000, {"EdDSA"}),      // a later clock: exp T0+600 is over
      profile("https://a.example/", {"client-a"}, T0, {"ES256"}),             // its EdDSA tokens fail the alg header
  };
  {
    std::vector<std::string> many;
    for (int k = 0; k < 17; ++k) many.push_back("aud-" + std::to_string(k));
    exps.push_back(profile("https://wide.example/", many, T0, {"EdDSA"}));   // no device slot
    exps.back().ExpirationLeeway = 5 * 1000000000LL;
  }
  const uint32_t kWide = 4;
  const std::string iss[] = {"https://a.example/", "https://b.example/", "https://c.example/", "https://a.example/",
                             "https://wide.example/"};
  const std::string aud[] = {"client-a", "client-b2", "client-c", "client-a", "aud-16"};
  auto payload = [&](const std::string& i, const std::string& a, int64_t exp, int k, const std::string& more = "") {
    return R"({"iss":")" + i + R"(","aud":[")" + a + R"(","other"],"exp":)" + std::to_string(exp) + R"(,"sub":"user-)" +
           std::to_string(k) + R"(","scope":"read write","roles":["r)" + std::to_string(k) + R"("],"n":)" +
           std::to_string(k) + ".5" + more + "}";
  };
  Batch b;
  for (int k = 0; k < 24; ++k) {
    for (uint32_t p = 0; p < 5; ++p) {                 // neighbouring tokens of different profiles
      const uint32_t o = (p + 1) % 3;                  // another tenant
      switch (k % 12) {
        case 0: case 1: case 2:
          b.add(p, payload(iss[p], aud[p], T0 + 1600, k));                    // valid for its own profile
          break;
        case 3: b.add(p, payload(iss[o], aud[p], T0 + 1600, k)); break;       // another tenant's issuer
        case 4: b.add(p, payload(iss[p], aud[o] + "x", T0 + 1600, k)); break;  // no audience of this profile
        case 5: b.add(p, payload(iss[p], aud[p], T0 + 600, k)); break;        // expired for profile 2's clock alone
        case 6: b.add(p, payload(iss[p], aud[p], T0 + 1600, k, R"(,"jti":"a\/b")")); break;   // an escape: the host path
        case 7: b.add(p, payload(iss[p], aud[p], T0 + 1600, k, R"(,"EXP":1)")); break;        // a field twice: the host path
        case 8: b.add(p, payload(iss[p], aud[p], T0 + 1600, k, R"(,"nbf":"soon")")); break;   // rejected on the host path
        case 9: b.add(p, payload(iss[p], aud[p], T0 + 1600, k), "ES256"); break;              // an alg only profiles 1 and 3 take
        case 10: b.add(p, payload(iss[p], aud[p], T0 - 600, k)); break;       // expired for all
        default: b.add(p, R"({"sub":"no dates"})"); break;
      }
    }
  }
  b.store.push_back("not-a-jwt");
  b.which.push_back(1);

  // 65 profiles in use: the last one finds no slot
  std::vector<Expected> many;
  Batch mb;
  for (int p = 0; p < 65; ++p) {
    const std::string i = "https://t" + std::to_string(p) + ".example/";
    many.push_back(profile(i, {"c" + std::to_string(p)}, T0 + p, {"EdDSA"}));
  }
  for (int k = 0; k < 3; ++k)
    for (int p = 0; p < 65; ++p) {
      const std::string i = "https://t" + std::to_string(k == 1 ? (p + 1) % 65 : p) + ".example/";
      mb.add((uint32_t)p, payload(i, "c" + std::to_string(p), T0 + 1600, k));
    }

  if (mode == "ok") {
    CheckStats st, sum;
    compare(*v, b, exps, "tenants", &st, &sum);
    check(each_stub_profiles == 4, "tenants: four profiles have a slot", std::to_string(each_stub_profiles));
    check(st.scanned == sum.scanned && st.host == sum.host && st.scanned > 0 && st.host > 0, "tenants: stats sum",
          std::to_string(st.scanned) + "+" + std::to_string(st.host) + " / " + std::to_string(sum.scanned) + "+" +
              std::to_string(sum.host));
    {
      // the wide profile's tokens took the host path, all of them that reached the claims
      const auto at = group(b, kWide);
      std::vector<std::string_view> part;
      for (size_t i : at) part.push_back(b.store[i]);
      CheckStats ws;
      const auto rs = v->CheckBatch(part, exps[kWide], &ws);
      check(ws.scanned == 0 && ws.host > 0 && rs[0].ok, "the 17-audience profile is not scannable", rs[0].err);
    }
    // expired for one profile only: the same payload under profiles 0 and 2
    {
      Batch two;
      const std::string pa = payload(iss[0], aud[0], T0 + 600, 1), pc = payload(iss[2], aud[2], T0 + 600, 1);
      two.add(0, pa);
      two.add(2, pc);
      const auto rs = v->CheckBatchEach(two.toks(), exps, two.which);
      check(rs[0].ok && !rs[1].ok && has(rs[1].err, "token is expired"), "expired for profile 2 alone", rs[1].err);
    }
    CheckStats mst, msum;
    compare(*v, mb, many, "65 profiles", &mst, &msum);
    check(each_stub_profiles == 64, "65 profiles: 64 slots", std::to_string(each_stub_profiles));
    check(mst.scanned == msum.scanned - 3 && mst.host == msum.host + 3 && msum.host == 0, "65 profiles: stats",
          std::to_string(mst.scanned) + "+" + std::to_string(mst.host));
    // a pool that runs over: profiles of 3000 bytes each, the third finds no room
    {
      std::vector<Expected> fat;
      Batch fb;
      for (int p = 0; p < 3; ++p) {
        const std::string i = "https://fat" + std::to_string(p) + ".example/" + std::string(3000, 'x');
        fat.push_back(profile(i, {}, T0, {"EdDSA"}));
        fb.add((uint32_t)p, payload(i, "any", T0 + 1600, p));
        fb.add((uint32_t)p, payload(i + "y", "any", T0 + 1600, p));
      }
      CheckStats fst, fsum;
      compare(*v, fb, fat, "pool", &fst, &fsum);
      check(each_stub_profiles == 2 && fst.scanned == 4 && fst.host == 2, "pool: two slots",
            std::to_string(each_stub_profiles) + " " + std::to_string(fst.scanned) + "+" + std::to_string(fst.host));
    }
    // one profile for all: the old entry
    {
      const std::vector<uint32_t> zeros(b.which.size(), 0);
      const auto a = v->CheckBatchEach(b.toks(), {exps[1]}, zeros);
      const auto w = v->CheckBatch(b.toks(), exps[1]);
      bool eq = a.size() == w.size();
      for (size_t i = 0; eq && i < a.size(); ++i) eq = a[i].ok == w[i].ok && a[i].err == w[i].err;
      check(eq, "one profile equals CheckBatch");
    }
    // the wall clock for a profile without Now
    {
      std::vector<Expected> e2 = {exps[0], exps[0]};
      e2[1].has_now = false;
      Batch two;
      two.add(0, payload(iss[0], aud[0], T0 + 1600, 1));
      two.add(1, payload(iss[0], aud[0], T0 + 1600, 1));
      const auto rs = v->CheckBatchEach(two.toks(), e2, two.which);
      check(rs[0].ok && !rs[1].ok && has(rs[1].err, "token is expired"), "Now is per profile", rs[1].err);
    }
    const auto toks = b.toks();
    check(throws_invalid([&] { v->CheckBatchEach(toks, exps, std::vector<uint32_t>(toks.size() - 1, 0)); }),
          "which.size() != tokens.size() throws");
    {
      auto w = b.which;
      w[7] = (uint32_t)exps.size();
      check(throws_invalid([&] { v->RegisteredBatchEach(toks, exps, w); }), "which[i] >= expected.size() throws");
      check(throws_invalid([&] { v->SelectBatchEach(toks, exps, w, kNames); }), "... in SelectBatchEach");
      check(throws_invalid([&] { v->CheckVerdictsEach(toks, exps, w); }), "... in CheckVerdictsEach");
    }
    check(throws_invalid([&] { v->CheckBatchEach(toks, {}, b.which); }), "no Expected with tokens throws");
    check(v->CheckBatchEach({}, {}, {}).empty() && v->SelectBatchEach({}, exps, {}, kNames).empty(), "empty batch");
  } else if (mode == "noeach") {
    const char* un = "capjwt: claims scan unavailable: capjwt: jg_claims_each: not provided by the loaded verifier library";
    const auto toks = b.toks();
    for (int round = 0; round < 2; ++round) {              // again after the context was recreated
      CheckStats st;
      const auto rs = v->CheckBatchEach(toks, exps, b.which, &st);
      const auto gs = v->RegisteredBatchEach(toks, exps, b.which);
      const auto ss = v->SelectBatchEach(toks, exps, b.which, kNames);
      size_t host_ok = 0, unavailable = 0;
      for (size_t i = 0; i < toks.size(); ++i) {
        const std::string at = "noeach: token " + std::to_string(i);
        if (i + 1 == toks.size()) {
          check(!rs[i].ok && !has(rs[i].err, "unavailable"), "noeach: parse error", rs[i].err);
        } else if (b.which[i] == kWide) {
          check(!has(rs[i].err, "unavailable"), at + " of the profile without a slot", rs[i].err);
          host_ok += rs[i].ok;
        } else {
          // a token that fails before the claims (an alg its key does not take) keeps that error
          const bool sig = has(rs[i].err, "error verifying token signature");
          check(!rs[i].ok && (rs[i].err == un || sig), at, rs[i].err);
          check(!gs[i].ok && gs[i].err == rs[i].err && !ss[i].ok && ss[i].err == rs[i].err && ss[i].values.empty(),
                at + " records", gs[i].err);
          unavailable += rs[i].err == un;
        }
      }
      check(unavailable > toks.size() / 2, "noeach: the scanned tokens are unavailable", std::to_string(unavailable));
      check(host_ok > 0 && st.scanned == 0 && st.host > 0, "noeach: the host path still answers");
    }
    const auto w = v->CheckBatch(toks, exps[0]);           // the old scan is there
    check(w[0].ok, "noeach: CheckBatch works", w[0].err);
  } else {
    std::printf("unknown mode %s\n", mode.c_str());
    return 2;
  }
  std::printf(fails ? "each %s: %d failures\n" : "each %s: ok\n", mode.c_str(), fails);
  return fails ? 1 : 0;
}
