// py_capjwt.cpp -- Python binding of the C++ cap jwt mirror (cap_jwt.hpp), so
// the parity tests can drive KeySet / Validator the way the reference's Go
// tests do (jwt/keyset_test.go, jwt/jwt_test.go).  Values cross as Go would
// hand them out: claims map -> dict with float64 numbers; error -> str or None.
#include <pybind11/functional.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>

#include "cap_jwt.hpp"

namespace py = pybind11;
using namespace capjwt;

namespace {

py::object to_py(const json::Value& v) {
  switch (v.kind) {
    case json::Value::Null: return py::none();
    case json::Value::Bool: return py::bool_(v.b);
    case json::Value::Number: return py::float_(v.num);
    case json::Value::String: return py::str(v.str.data(), v.str.size());
    case json::Value::Array: {
      py::list l;
      for (const auto& e : v.arr) l.append(to_py(e));
      return std::move(l);
    }
    case json::Value::Object: {
      py::dict d;
      for (const auto& m : v.obj) d[py::str(m.first)] = to_py(m.second);
      return std::move(d);
    }
  }
  return py::none();
}

py::tuple result_py(const Result& r) {
  if (r.ok) return py::make_tuple(to_py(r.claims), py::none());
  return py::make_tuple(py::none(), py::str(r.err));
}

// go-jose's jwt.Claims of an accepted token as RegisteredBatch / SelectBatch return it
py::dict claims_py(const RegisteredClaims& c) {
  auto date = [](const std::optional<int64_t>& d) -> py::object {
    return d ? py::object(py::int_(*d)) : py::object(py::none());
  };
  py::dict d;
  d["iss"] = py::str(c.Issuer);
  d["sub"] = py::str(c.Subject);
  d["jti"] = py::str(c.ID);
  py::list aud;
  for (const auto& a : c.Audience) aud.append(py::str(a));
  d["aud"] = aud;
  d["exp"] = date(c.Expiry);
  d["nbf"] = date(c.NotBefore);
  d["iat"] = date(c.IssuedAt);
  return d;
}

// a bytes object the host threads write into: nothing is copied afterwards
py::bytes fresh_bytes(size_t bytes) {
  PyObject* o = PyBytes_FromStringAndSize(nullptr, (Py_ssize_t)bytes);
  if (!o) throw py::error_already_set();
  return py::reinterpret_steal<py::bytes>(o);
}
void* bytes_mem(py::bytes& b) { return (void*)PyBytes_AS_STRING(b.ptr()); }

// RegisteredColumns over bytes objects (RegisteredBlob, SelectBlob)
struct RegisteredBlobCols {
  py::bytes ok, present, exp, nbf, iat;
  py::bytes off[4];
  py::bytes var[5];
  RegisteredColumns R;
  explicit RegisteredBlobCols(size_t n)
      : ok(fresh_bytes(n)), present(fresh_bytes(n)), exp(fresh_bytes(8 * n)), nbf(fresh_bytes(8 * n)),
        iat(fresh_bytes(8 * n)),
        off{fresh_bytes(4 * (n + 1)), fresh_bytes(4 * (n + 1)), fresh_bytes(4 * (n + 1)), fresh_bytes(4 * (n + 1))} {
    R.ok = (uint8_t*)bytes_mem(ok);
    R.present = (uint8_t*)bytes_mem(present);
    R.exp = (int64_t*)bytes_mem(exp);
    R.nbf = (int64_t*)bytes_mem(nbf);
    R.iat = (int64_t*)bytes_mem(iat);
    R.iss_off = (uint32_t*)bytes_mem(off[0]);
    R.sub_off = (uint32_t*)bytes_mem(off[1]);
    R.jti_off = (uint32_t*)bytes_mem(off[2]);
    R.aud_tok = (uint32_t*)bytes_mem(off[3]);
    R.alloc = [this](RegisteredColumns::Var which, size_t bytes) {
      py::gil_scoped_acquire gil;
      var[which] = fresh_bytes(bytes);
      return bytes_mem(var[which]);
    };
  }
  RegisteredBlobCols(const RegisteredBlobCols&) = delete;
  RegisteredBlobCols& operator=(const RegisteredBlobCols&) = delete;
  py::dict dict() {
    py::dict d;
    d["ok"] = ok;
    d["present"] = present;
    d["exp"] = exp;
    d["nbf"] = nbf;
    d["iat"] = iat;
    d["iss"] = py::make_tuple(off[0], var[RegisteredColumns::ISS]);
    d["sub"] = py::make_tuple(off[1], var[RegisteredColumns::SUB]);
    d["jti"] = py::make_tuple(off[2], var[RegisteredColumns::JTI]);
    d["aud"] = py::make_tuple(off[3], var[RegisteredColumns::AUD_OFF], var[RegisteredColumns::AUD]);
    return d;
  }
};

py::list results_py(const Results& rs) {
  py::list l;
  for (const auto& r : rs) l.append(result_py(r));
  return l;
}

std::vector<std::string> as_strings(const py::sequence& toks) {
  std::vector<std::string> v;
  v.reserve(py::len(toks));
  for (auto t : toks) {
    if (py::isinstance<py::bytes>(t)) v.push_back(t.cast<std::string>());
    else v.push_back(t.cast<std::string>());
  }
  return v;
}

std::vector<std::string_view> views(const std::vector<std::string>& s) {
  return std::vector<std::string_view>(s.begin(), s.end());
}

// newline-separated token blob -> views (end-to-end benchmark input, no
// per-token Python objects).  One thread: a parallel split measured 4-5x
// slower on the GPU box (16-CPU cgroup quota: a 16-thread burst next to the
// runtime's own threads is throttled for the rest of the CFS period).
void split_range(const char* p, const char* end, std::vector<std::string_view>& v) {
  while (p < end) {
    const char* nl = static_cast<const char*>(std::memchr(p, '\n', (size_t)(end - p)));
    const char* e = nl ? nl : end;
    if (e > p) v.emplace_back(p, (size_t)(e - p));
    p = e + 1;
  }
}

// newline-separated tokens -> views; a large blob is cut at newlines into one
// range per host thread (a 1M-token blob: 9 ms on one thread)
std::vector<std::string_view> split_lines(const char* p, size_t n) {
  const size_t th = n >= (size_t(64) << 20) ? (size_t)capjwt::host_threads() : 1;
  std::vector<const char*> cut{p};
  for (size_t t = 1; t < th; ++t) {
    const char* c = p + n * t / th;
    const char* nl = static_cast<const char*>(std::memchr(c, '\n', (size_t)(p + n - c)));
    cut.push_back(nl && nl + 1 > cut.back() ? nl + 1 : cut.back());
  }
  cut.push_back(p + n);
  std::vector<std::vector<std::string_view>> part(cut.size() - 1);
  auto run = [&](size_t k) {
    part[k].reserve((size_t)(cut[k + 1] - cut[k]) / 256 + 1);
    split_range(cut[k], cut[k + 1], part[k]);
  };
  std::vector<std::thread> ths;
  for (size_t k = 1; k < part.size(); ++k) ths.emplace_back(run, k);
  run(0);
  for (auto& t : ths) t.join();
  if (part.size() == 1) return std::move(part[0]);
  size_t total = 0;
  for (auto& x : part) total += x.size();
  std::vector<std::string_view> v;
  v.reserve(total);
  for (auto& x : part) v.insert(v.end(), x.begin(), x.end());
  return v;
}

Fetcher wrap_fetch(py::object fn) {
  // fn(url, ca_pem) -> dict(status=, status_text=, body=, content_type=, max_age=); raise = transport error
  auto holder = std::make_shared<py::object>(std::move(fn));
  return [holder](const std::string& url, const std::string& ca) -> FetchResponse {
    py::gil_scoped_acquire g;
    FetchResponse r;
    py::object res;
    try {
      res = (*holder)(url, ca);
    } catch (py::error_already_set& e) {
      throw std::runtime_error(std::string("Get \"") + url + "\": " + e.what());
    }
    py::dict d = res.cast<py::dict>();
    if (d.contains("status")) r.status = d["status"].cast<int>();
    r.status_text = d.contains("status_text") ? d["status_text"].cast<std::string>()
                                              : std::to_string(r.status) + (r.status == 200 ? " OK" : "");
    if (d.contains("body")) {
      py::object b = d["body"];
      r.body = py::isinstance<py::bytes>(b) ? b.cast<std::string>() : b.cast<std::string>();
    }
    if (d.contains("content_type")) r.content_type = d["content_type"].cast<std::string>();
    if (d.contains("max_age")) r.max_age_s = d["max_age"].cast<int64_t>();
    return r;
  };
}

struct PyKeySet {
  std::shared_ptr<KeySet> ks;
};

PyKeySet must(std::unique_ptr<KeySet> p, const std::string& err) {
  if (!p) throw py::value_error(err);
  return PyKeySet{std::shared_ptr<KeySet>(std::move(p))};
}

py::dict key_dict(const PublicKey& k) {
  py::dict d;
  static const char* kinds[] = {"none", "RSA", "EC", "Ed25519", "oct"};
  d["kind"] = kinds[k.kind];
  if (k.kind == PublicKey::RSA) {
    d["n"] = py::bytes(k.n);
    d["e"] = k.e;
  } else if (k.kind == PublicKey::EC) {
    static const char* crv[] = {"", "P-256", "P-384", "P-521"};
    d["crv"] = crv[k.curve];
    d["x"] = py::bytes(k.x);
    d["y"] = py::bytes(k.y);
  } else if (k.kind == PublicKey::Ed25519) {
    d["x"] = py::bytes(k.x);
  } else if (k.kind == PublicKey::Symmetric) {
    d["k"] = py::bytes(k.k);
  }
  return d;
}

// the per-token profile indices of a *_blob_each call: any C-contiguous buffer of uint32
std::vector<uint32_t> which_of(const py::buffer& b) {
  const py::buffer_info info = b.request();
  if (info.itemsize != 4 || (info.format != py::format_descriptor<uint32_t>::format() && info.format != "L" &&
                             info.format != "=I" && info.format != "<I"))
    throw py::value_error("which must be a buffer of uint32");
  if (info.ndim != 1 || (info.size > 0 && info.strides[0] != 4))
    throw py::value_error("which must be contiguous, one dimension");
  const uint32_t* p = (const uint32_t*)info.ptr;
  return std::vector<uint32_t>(p, p + info.size);
}

// A column of n int64 operands (MatchBatchArgs' nums): any contiguous buffer of int64
const int64_t* int64_column(const py::buffer_info& info, size_t n) {
  if (info.itemsize != 8 || (info.format != "q" && info.format != "l" && info.format != "=q" && info.format != "<q"))
    throw py::value_error("a number column must be a buffer of int64");
  if (info.ndim != 1 || (info.size > 0 && info.strides[0] != 8))
    throw py::value_error("a number column must be contiguous, one dimension");
  if ((size_t)info.size != n) throw py::value_error("a number column does not hold one operand per token");
  return (const int64_t*)info.ptr;
}

// A column of string operands as newline-separated bytes (MatchBlobArgs' strs): every piece between newlines is
// an operand, empty ones too.  One newline after the last operand is allowed: an empty piece beyond the one per
// token is dropped.
std::vector<std::string_view> split_operands(const char* p, size_t n, size_t ntokens) {
  std::vector<std::string_view> v;
  v.reserve(ntokens + 1);
  const char* const end = p + n;
  for (;;) {
    const char* nl = static_cast<const char*>(std::memchr(p, '\n', (size_t)(end - p)));
    const char* e = nl ? nl : end;
    v.emplace_back(p, (size_t)(e - p));
    if (!nl) break;
    p = nl + 1;
  }
  if (v.size() == ntokens + 1 && v.back().empty()) v.pop_back();
  return v;
}

}  // namespace

PYBIND11_MODULE(_capjwt_host, m) {
  m.doc() = "C++ host mirror of cap's jwt package over the MI355X verifier (libcapjwt.so)";

  py::class_<PublicKey>(m, "PublicKey")
      .def_static("rsa", [](py::bytes n, uint64_t e) {
        PublicKey k;
        k.kind = PublicKey::RSA;
        std::string s = n;
        size_t i = 0;
        while (i < s.size() && s[i] == 0) ++i;
        k.n = s.substr(i);
        k.e = e;
        return k;
      })
      .def_static("ec", [](const std::string& crv, py::bytes x, py::bytes y) {
        PublicKey k;
        k.kind = PublicKey::EC;
        k.curve = crv == "P-256" ? 1 : crv == "P-384" ? 2 : crv == "P-521" ? 3 : 0;
        if (!k.curve) throw py::value_error("unsupported curve " + crv);
        k.x = x;
        k.y = y;
        return k;
      })
      .def_static("ed25519", [](py::bytes pub) {
        PublicKey k;
        k.kind = PublicKey::Ed25519;
        k.x = pub;
        return k;
      })
      .def_static("symmetric", [](py::bytes secret) {
        PublicKey k;
        k.kind = PublicKey::Symmetric;
        k.k = secret;
        return k;
      })
      .def("as_dict", &key_dict)
      .def("__eq__", [](const PublicKey& a, const PublicKey& b) { return a == b; });

  py::class_<Expected>(m, "Expected")
      .def(py::init<>())
      .def_readwrite("Issuer", &Expected::Issuer)
      .def_readwrite("Subject", &Expected::Subject)
      .def_readwrite("ID", &Expected::ID)
      .def_readwrite("Audiences", &Expected::Audiences)
      .def_readwrite("SigningAlgorithms", &Expected::SigningAlgorithms)
      .def_readwrite("NotBeforeLeeway", &Expected::NotBeforeLeeway)
      .def_readwrite("ExpirationLeeway", &Expected::ExpirationLeeway)
      .def_readwrite("ClockSkewLeeway", &Expected::ClockSkewLeeway)
      .def_readwrite("has_now", &Expected::has_now)
      .def_readwrite("now_unix_ns", &Expected::now_unix_ns);

  // ---- CPU-side pieces (no GPU needed)
  m.def("supported_signing_algorithm", [](const std::vector<std::string>& algs) -> py::object {
    const std::string e = SupportedSigningAlgorithm(algs);
    if (e.empty()) return py::none();
    return py::str(e);
  });
  m.def("json_loads", [](py::bytes b) -> py::tuple {
    json::Value v;
    std::string err;
    std::string s = b;
    if (!json::parse(s, &v, &err)) return py::make_tuple(py::none(), py::str(err));
    if (json::has_range_error(v)) return py::make_tuple(py::none(), py::str("number out of range"));
    return py::make_tuple(to_py(v), py::none());
  });
  m.def("json_marshal", [](py::bytes b) -> py::object {
    // json.Marshal of the parsed interface{} (sorted keys; a member appears once)
    json::Value v;
    std::string err, s = b;
    if (!json::parse(s, &v, &err)) return py::none();
    return py::bytes(json::marshal(v));
  });
  m.def("b64url_decode", [](const std::string& s) -> py::object {
    std::string out, err;
    if (!b64url_decode(s, &out, &err)) return py::none();
    return py::bytes(out);
  });
  m.def("strip_whitespace", [](py::bytes s) { return py::bytes(strip_whitespace(std::string(s))); });
  m.def("parse_signed", [](py::bytes tok) -> py::dict {
    JWS j;
    std::string err;
    py::dict d;
    std::string t = tok;
    if (!parse_signed(t, &j, &err)) {
      d["error"] = err;
      return d;
    }
    d["error"] = py::none();
    d["payload"] = py::bytes(j.payload);
    d["nsigs"] = j.sigs.size();
    if (!j.sigs.empty()) {
      d["alg"] = j.sigs[0].alg;
      d["kid"] = j.sigs[0].kid;
      d["signature"] = py::bytes(j.sigs[0].signature);
      d["protected"] = py::bytes(j.sigs[0].protected_raw);
    }
    std::string si;
    if (signing_input(j, &si)) d["signing_input"] = py::bytes(si);
    else d["signing_input"] = py::none();
    return d;
  });
  m.def("parse_public_key_pem", [](py::bytes pem) {
    PublicKey k;
    std::string err;
    if (!ParsePublicKeyPEM(std::string(pem), &k, &err)) throw py::value_error(err);
    return k;
  });
  m.def("jwks_decode", [](py::bytes doc) {
    std::vector<JSONWebKey> keys;
    std::string err;
    if (!jwks_decode(std::string(doc), &keys, &err)) throw py::value_error(err);
    py::list l;
    for (const auto& k : keys) l.append(py::make_tuple(k.kid, k.key));
    return l;
  });
  m.def("ec_on_curve", [](const std::string& crv, py::bytes x, py::bytes y) {
    const int c = crv == "P-256" ? 1 : crv == "P-384" ? 2 : crv == "P-521" ? 3 : 0;
    return ec_on_curve(c, std::string(x), std::string(y));
  });
  m.def("validate_claims", [](py::bytes payload, const std::string& alg, size_t sig_len, const Expected& exp,
                              int64_t now_ns) {
    // the post-signature half of Validate on a payload whose signature verified
    json::Value v;
    std::string err;
    if (!json::parse(std::string(payload), &v, &err)) return py::tuple(py::make_tuple(py::none(), py::str(err)));
    TokenInfo info;
    info.parsed = true;
    info.nsigs = 1;
    info.sig0_len = sig_len;
    info.alg = alg;
    Result r = validate_claims(v, info, exp, now_ns);
    if (r.ok) r.claims = v;
    return result_py(r);
  });
  m.def("match_requires", [](py::bytes payload, const std::vector<std::tuple<ClaimPath, int, std::string>>& reqs) {
    // the host path of MatchBatch on a payload whose claims were accepted: the mask
    json::Value v;
    std::string err;
    if (!json::parse(std::string(payload), &v, &err)) throw py::value_error(err);
    std::vector<Require> rq;
    for (const auto& [path, op, value] : reqs) rq.push_back(Require{path, (Require::Op)op, value});
    return match_requires(v, rq);
  });
  m.def("match_requires_args", [](py::bytes payload,
                                  const std::vector<std::tuple<ClaimPath, int, std::string, int64_t, uint32_t>>& reqs,
                                  const std::vector<std::string>& strs, const std::vector<int64_t>& nums) {
    // the host path of MatchBatchArgs with one token's operands: the mask
    json::Value v;
    std::string err;
    if (!json::parse(std::string(payload), &v, &err)) throw py::value_error(err);
    std::vector<Require> rq;
    for (const auto& [path, op, value, bound, column] : reqs)
      rq.push_back(Require{path, (Require::Op)op, value, bound, column});
    try {
      return match_requires(v, rq, std::vector<std::string_view>(strs.begin(), strs.end()), nums);
    } catch (const std::invalid_argument& e) {
      throw py::value_error(e.what());
    }
  });
  m.def("match_requires_hash", [](py::bytes payload,
                                  const std::vector<std::tuple<ClaimPath, int, std::string, int64_t, uint32_t>>& reqs,
                                  const std::vector<std::string>& strs, const std::vector<int64_t>& nums,
                                  const std::vector<std::optional<py::bytes>>& hashed) {
    // the host path of MatchBatchArgs with one token's operands and its hash columns, already hashed
    // and encoded (None: no value): the mask
    json::Value v;
    std::string err;
    if (!json::parse(std::string(payload), &v, &err)) throw py::value_error(err);
    std::vector<Require> rq;
    for (const auto& [path, op, value, bound, column] : reqs)
      rq.push_back(Require{path, (Require::Op)op, value, bound, column});
    std::vector<std::optional<std::string>> hx;
    for (const auto& h : hashed) hx.push_back(h ? std::optional<std::string>(std::string(*h)) : std::nullopt);
    try {
      return match_requires(v, rq, std::vector<std::string_view>(strs.begin(), strs.end()), nums, hx);
    } catch (const std::invalid_argument& e) {
      throw py::value_error(e.what());
    }
  });
  m.def("host_threads", &host_threads);
  m.def("set_host_memory_retention", &SetHostMemoryRetention);
  m.def("trim_host_memory", &TrimHostMemory);
  m.def("host_memory_retained", &HostMemoryRetained);
  m.def("available_cpus", &available_cpus);

  // ---- GPU-backed key sets and validator
  py::class_<PyKeySet>(m, "KeySet")
      .def("verify_signature", [](PyKeySet& s, py::object tok) {
        std::string t = tok.cast<std::string>();
        Result r;
        {
          py::gil_scoped_release rel;
          r = s.ks->VerifySignature(t);
        }
        return result_py(r);
      })
      .def("verify_signature_batch", [](PyKeySet& s, py::sequence toks) {
        auto v = as_strings(toks);
        Results rs;
        {
          py::gil_scoped_release rel;
          rs = s.ks->VerifySignatureBatch(views(v));
        }
        return results_py(rs);
      })
      .def("wait_tables", [](PyKeySet& s) {
        py::gil_scoped_release rel;
        s.ks->WaitTables();
      })
      .def("set_coalescing", [](PyKeySet& s, int max_inflight, size_t max_batch, int64_t window_us) {
        CoalesceConfig c;
        c.max_inflight = max_inflight;
        c.max_batch = max_batch;
        c.window_us = window_us;
        s.ks->SetCoalescing(c);
      }, py::arg("max_inflight") = 2, py::arg("max_batch") = 65536, py::arg("window_us") = 0)
      .def("coalescing_stats", [](PyKeySet& s) {
        const auto st = s.ks->CoalescingStats();
        py::dict d;
        d["calls"] = st.calls;
        d["batches"] = st.batches;
        d["max_batch"] = st.max_batch_seen;
        return d;
      })
      .def("device_status", [](PyKeySet& s) {
        py::gil_scoped_release rel;
        return s.ks->DeviceStatus();
      })
      .def("device_recoveries", [](PyKeySet& s) { return s.ks->DeviceRecoveries(); })
      .def("_debug_fail_verify", [](PyKeySet& s, int n) {
        if (s.ks->DebugFailVerify(n) != 0) throw py::value_error("jg_debug_fail_verify failed");
      });

  m.def("new_static_keyset", [](const std::vector<PublicKey>& keys, const std::vector<int>& devices) {
    std::string err;
    return must(NewStaticKeySet(keys, &err, devices), err);
  }, py::arg("keys"), py::arg("devices") = std::vector<int>{});
  m.def("new_json_web_keyset", [](const std::string& url, const std::string& ca, py::object fetch,
                                  const std::vector<int>& devices) {
    std::string err;
    return must(NewJSONWebKeySet(url, ca, wrap_fetch(std::move(fetch)), &err, devices), err);
  }, py::arg("url"), py::arg("ca_pem"), py::arg("fetch"), py::arg("devices") = std::vector<int>{});
  m.def("new_oidc_discovery_keyset", [](const std::string& issuer, const std::string& ca, py::object fetch,
                                        const std::vector<int>& devices) {
    std::string err;
    std::unique_ptr<KeySet> ks;
    {
      ks = NewOIDCDiscoveryKeySet(issuer, ca, wrap_fetch(std::move(fetch)), &err, devices);
    }
    return must(std::move(ks), err);
  }, py::arg("issuer"), py::arg("ca_pem"), py::arg("fetch"), py::arg("devices") = std::vector<int>{});

  struct PyValidator {
    std::shared_ptr<KeySet> ks;
    std::unique_ptr<Validator> v;
  };
  // check_batch .. select_blob below, once for one Expected (e) and once for an
  // Expected per token (es[w[i]]): the *_each bindings
  struct Who {
    const Expected* e;
    const std::vector<Expected>* es;
    const std::vector<uint32_t>* w;
  };
  auto py_check_batch = [](PyValidator& s, py::sequence toks, const Who& who) {
    // verdict only: (list of error strings or None, tokens the device's
    // claims scan decided, tokens that took the host claims path)
    auto v = as_strings(toks);
    std::vector<CheckResult> rs;
    CheckStats st;
    {
      py::gil_scoped_release rel;
      rs = who.es ? s.v->CheckBatchEach(views(v), *who.es, *who.w, &st) : s.v->CheckBatch(views(v), *who.e, &st);
    }
    py::list out(rs.size());
    for (size_t i = 0; i < rs.size(); ++i) {
      if (rs[i].ok) out[i] = py::none();
      else out[i] = py::str(rs[i].err);
    }
    return py::make_tuple(out, st.scanned, st.host);
  };
  auto py_check_blob = [](PyValidator& s, py::bytes blob, const Who& who) {
    // validate_blob's verdict-only twin: newline-separated tokens in,
    // (accept bytes, scanned, host) out
    char* bp = nullptr;
    Py_ssize_t bn = 0;
    if (PyBytes_AsStringAndSize(blob.ptr(), &bp, &bn) != 0) throw py::error_already_set();
    std::string ok;
    CheckStats st;
    {
      py::gil_scoped_release rel;
      const bool trace = std::getenv("CAPJWT_TRACE") != nullptr;
      auto t0 = std::chrono::steady_clock::now();
      auto lap = [&](const char* what) {
        if (!trace) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[capjwt] cblob %-12s %8.2f ms\n", what,
                     std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
      };
      auto toks = split_lines(bp, (size_t)bn);
      lap("split");
      const auto rs = who.es ? s.v->CheckVerdictsEach(toks, *who.es, *who.w, &st)
                             : s.v->CheckVerdicts(toks, *who.e, &st);
      lap("check");
      ok.assign((const char*)rs.data(), rs.size());
      lap("verdicts");
    }
    return py::make_tuple(py::bytes(ok), st.scanned, st.host);
  };
  auto py_registered_batch = [](PyValidator& s, py::sequence toks, const Who& who) {
    // check_batch with jwt.Claims: ([(claims dict or None, error or None)], scanned, host)
    auto v = as_strings(toks);
    std::vector<RegisteredResult> rs;
    CheckStats st;
    {
      py::gil_scoped_release rel;
      rs = who.es ? s.v->RegisteredBatchEach(views(v), *who.es, *who.w, &st)
                  : s.v->RegisteredBatch(views(v), *who.e, &st);
    }
    py::list out(rs.size());
    for (size_t i = 0; i < rs.size(); ++i) {
      if (!rs[i].ok) out[i] = py::make_tuple(py::none(), py::str(rs[i].err));
      else out[i] = py::make_tuple(claims_py(rs[i].claims), py::none());
    }
    return py::make_tuple(out, st.scanned, st.host);
  };
  auto py_registered_blob = [](PyValidator& s, py::bytes blob, const Who& who) {
    // check_blob with the registered claims as columns: newline-separated
    // tokens in, (dict of bytes, scanned, host) out -- no per-token object
    char* bp = nullptr;
    Py_ssize_t bn = 0;
    if (PyBytes_AsStringAndSize(blob.ptr(), &bp, &bn) != 0) throw py::error_already_set();
    const bool trace = std::getenv("CAPJWT_TRACE") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
      if (!trace) return;
      const auto t1 = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[capjwt] rblob %-12s %8.2f ms\n", what,
                   std::chrono::duration<double, std::milli>(t1 - t0).count());
      t0 = t1;
    };
    auto toks = split_lines(bp, (size_t)bn);
    lap("split");
    // the columns are bytes objects from the start
    RegisteredBlobCols C(toks.size());
    CheckStats st;
    {
      py::gil_scoped_release rel;
      if (who.es) s.v->RegisteredColsEach(toks, *who.es, *who.w, C.R, &st);
      else s.v->RegisteredCols(toks, *who.e, C.R, &st);
    }
    lap("registered");
    return py::make_tuple(C.dict(), st.scanned, st.host);
  };
  using PathList = std::vector<ClaimPath>;
  // a name list as it is, a path list as the ClaimPaths the path overloads take
  struct AsKeys {
    const std::vector<std::string>& operator()(const std::vector<std::string>& names) const { return names; }
    ClaimPaths operator()(const PathList& paths) const { return ClaimPaths{paths}; }
  };
  auto py_select_batch = [](PyValidator& s, py::sequence toks, const auto& names, const Who& who) {
    // registered_batch with the claims `names` name:
    // ([(claims dict or None, {name: value} or None, error or None)], scanned, host);
    // for a list of paths the values are keyed by the path's index in it
    auto v = as_strings(toks);
    std::vector<SelectResult> rs;
    CheckStats st;
    {
      py::gil_scoped_release rel;
      rs = who.es ? s.v->SelectBatchEach(views(v), *who.es, *who.w, AsKeys{}(names), &st)
                  : s.v->SelectBatch(views(v), *who.e, AsKeys{}(names), &st);
    }
    py::list out(rs.size());
    for (size_t i = 0; i < rs.size(); ++i) {
      if (!rs[i].ok) {
        out[i] = py::make_tuple(py::none(), py::none(), py::str(rs[i].err));
        continue;
      }
      py::dict vals;
      for (size_t k = 0; k < names.size(); ++k)
        if (rs[i].values[k]) {
          if constexpr (std::is_same_v<std::decay_t<decltype(names)>, PathList>) vals[py::int_(k)] = to_py(*rs[i].values[k]);
          else vals[py::str(names[k])] = to_py(*rs[i].values[k]);
        }
      out[i] = py::make_tuple(claims_py(rs[i].claims), vals, py::none());
    }
    return py::make_tuple(out, st.scanned, st.host);
  };
  auto py_select_blob = [](PyValidator& s, py::bytes blob, const auto& names, const Who& who) {
    // registered_blob with, per name, the value's type / number / text columns
    char* bp = nullptr;
    Py_ssize_t bn = 0;
    if (PyBytes_AsStringAndSize(blob.ptr(), &bp, &bn) != 0) throw py::error_already_set();
    const bool trace = std::getenv("CAPJWT_TRACE") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
      if (!trace) return;
      const auto t1 = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[capjwt] sblob %-12s %8.2f ms\n", what,
                   std::chrono::duration<double, std::milli>(t1 - t0).count());
      t0 = t1;
    };
    auto toks = split_lines(bp, (size_t)bn);
    lap("split");
    const size_t n = toks.size();
    RegisteredBlobCols C(n);
    std::vector<py::bytes> type(names.size()), num(names.size()), text_off(names.size()), text(names.size());
    SelectColumns S;
    S.reg = C.R;
    S.names.resize(names.size());
    for (size_t k = 0; k < names.size(); ++k) {
      type[k] = fresh_bytes(n);
      num[k] = fresh_bytes(8 * n);
      text_off[k] = fresh_bytes(4 * (n + 1));
      S.names[k].type = (uint8_t*)bytes_mem(type[k]);
      S.names[k].num = (double*)bytes_mem(num[k]);
      S.names[k].text_off = (uint32_t*)bytes_mem(text_off[k]);
    }
    S.alloc_text = [&](size_t k, size_t bytes) {
      py::gil_scoped_acquire gil;
      text[k] = fresh_bytes(bytes);
      return bytes_mem(text[k]);
    };
    CheckStats st;
    {
      py::gil_scoped_release rel;
      if (who.es) s.v->SelectColsEach(toks, *who.es, *who.w, AsKeys{}(names), S, &st);
      else s.v->SelectCols(toks, *who.e, AsKeys{}(names), S, &st);
    }
    lap("select");
    py::dict d = C.dict();
    py::list sel;
    for (size_t k = 0; k < names.size(); ++k) {
      py::dict c;
      c["type"] = type[k];
      c["num"] = num[k];
      c["text_off"] = text_off[k];
      c["text"] = text[k];
      sel.append(c);
    }
    d["sel"] = sel;
    return py::make_tuple(d, st.scanned, st.host);
  };
  // a requirement as Python hands it over: (path, op, value)
  using ReqList = std::vector<std::tuple<ClaimPath, int, std::string>>;
  auto requires_of = [](const ReqList& reqs) {
    std::vector<Require> rq;
    rq.reserve(reqs.size());
    for (const auto& [path, op, value] : reqs) rq.push_back(Require{path, (Require::Op)op, value});
    return rq;
  };
  auto py_match_batch = [=](PyValidator& s, py::sequence toks, const ReqList& reqs, const Who& who) {
    // check_batch with the requirements' mask: ([(bits or None, error or None)], scanned, host)
    auto v = as_strings(toks);
    const std::vector<Require> rq = requires_of(reqs);
    std::vector<MatchResult> rs;
    CheckStats st;
    {
      py::gil_scoped_release rel;
      rs = who.es ? s.v->MatchBatchEach(views(v), *who.es, *who.w, rq, &st) : s.v->MatchBatch(views(v), *who.e, rq, &st);
    }
    py::list out(rs.size());
    for (size_t i = 0; i < rs.size(); ++i) {
      if (rs[i].ok) out[i] = py::make_tuple(py::int_(rs[i].bits), py::none());
      else out[i] = py::make_tuple(py::none(), py::str(rs[i].err));
    }
    return py::make_tuple(out, st.scanned, st.host);
  };
  auto py_match_blob = [=](PyValidator& s, py::bytes blob, const ReqList& reqs, const Who& who) {
    // check_blob with a uint32 mask column: newline-separated tokens in,
    // ({"ok": accept bytes, "match": masks}, scanned, host) out -- no strings
    char* bp = nullptr;
    Py_ssize_t bn = 0;
    if (PyBytes_AsStringAndSize(blob.ptr(), &bp, &bn) != 0) throw py::error_already_set();
    const std::vector<Require> rq = requires_of(reqs);
    const bool trace = std::getenv("CAPJWT_TRACE") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
      if (!trace) return;
      const auto t1 = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[capjwt] mblob %-12s %8.2f ms\n", what,
                   std::chrono::duration<double, std::milli>(t1 - t0).count());
      t0 = t1;
    };
    auto toks = split_lines(bp, (size_t)bn);
    lap("split");
    py::bytes ok = fresh_bytes(toks.size()), match = fresh_bytes(4 * toks.size());
    uint8_t* const okp = (uint8_t*)bytes_mem(ok);
    uint32_t* const mp = (uint32_t*)bytes_mem(match);
    CheckStats st;
    {
      py::gil_scoped_release rel;
      if (who.es) s.v->MatchVerdictsEach(toks, *who.es, *who.w, rq, okp, mp, &st);
      else s.v->MatchVerdicts(toks, *who.e, rq, okp, mp, &st);
    }
    lap("match");
    py::dict d;
    d["ok"] = ok;
    d["match"] = match;
    return py::make_tuple(d, st.scanned, st.host);
  };
  // a requirement of the MatchArgs entries: (path, op, value, bound, column)
  using ArgReqList = std::vector<std::tuple<ClaimPath, int, std::string, int64_t, uint32_t>>;
  auto arg_requires_of = [](const ArgReqList& reqs) {
    std::vector<Require> rq;
    rq.reserve(reqs.size());
    for (const auto& [path, op, value, bound, column] : reqs) {
      rq.push_back(Require{path, (Require::Op)op, value, bound, column});
      // InSet / AnyElementIn: the column is the handle's token (ClaimSet.token)
      if (op == Require::InSet || op == Require::AnyElementIn) {
        rq.back().set = ClaimSet::from_token(column);
        if (!rq.back().set) throw py::value_error("capjwt: the claim set of a requirement is gone");
        rq.back().column = 0;
      }
    }
    return rq;
  };
  struct PyClaimSet {
    std::shared_ptr<KeySet> ks;     // the context the set lives in
    ClaimSet set;
  };
  py::class_<PyClaimSet>(m, "ClaimSet")
      .def("replace", [](PyClaimSet& s, const std::vector<std::string>& members, std::optional<uint32_t> seed) {
        py::gil_scoped_release rel;
        s.set.Replace(members, seed);
      }, py::arg("members"), py::arg("seed") = py::none())
      .def("add", [](PyClaimSet& s, const std::vector<std::string>& members) {
        py::gil_scoped_release rel;
        return s.set.Add(members);
      }, py::arg("members"))
      .def("close", [](PyClaimSet& s) { s.set.Close(); })
      .def("token", [](PyClaimSet& s) { return s.set.token(); })
      .def("__len__", [](PyClaimSet& s) { return s.set.size(); })
      .def("info", [](PyClaimSet& s) {
        const ClaimSet::Info i = s.set.info();
        py::dict d;
        d["n"] = i.n;
        d["host_only"] = i.host_only;
        d["nslots"] = i.nslots;
        d["maxprobe"] = i.maxprobe;
        d["seed"] = i.seed;
        d["pool_bytes"] = i.pool_bytes;
        d["generation"] = i.generation;
        return d;
      });
  // the number columns of a call: the buffers stay requested (and so alive) for its duration
  struct NumCols {
    std::vector<py::buffer_info> infos;
    std::vector<const int64_t*> cols;
    NumCols(const std::vector<py::buffer>& nums, size_t n) {
      for (const py::buffer& b : nums) {
        infos.push_back(b.request());
        cols.push_back(int64_column(infos.back(), n));
      }
    }
  };
  // The hash columns of a batch call: an entry is bytes or str (the value to hash) or None.  The texts are
  // copied out while the GIL is held; the views point into the copies.
  struct HashCols {
    std::vector<std::vector<std::string>> store;
    std::vector<HashColumn> cols;
    explicit HashCols(const std::vector<py::sequence>& hashes) {
      store.resize(hashes.size());
      cols.resize(hashes.size());
      for (size_t c = 0; c < hashes.size(); ++c) {
        const size_t n = (size_t)py::len(hashes[c]);
        store[c].resize(n);
        cols[c].resize(n);
        std::vector<uint8_t> has(n, 0);
        for (size_t i = 0; i < n; ++i) {
          py::object o = hashes[c][i];
          if (o.is_none()) continue;
          if (!py::isinstance<py::bytes>(o) && !py::isinstance<py::str>(o))
            throw py::type_error("a hash column holds bytes, str or None");
          store[c][i] = o.cast<std::string>();
          has[i] = 1;
        }
        for (size_t i = 0; i < n; ++i)
          if (has[i]) cols[c][i] = std::string_view(store[c][i]);
      }
    }
  };
  auto py_match_batch_args = [=](PyValidator& s, py::sequence toks, const ArgReqList& reqs,
                                 const std::vector<std::vector<std::string>>& strs, const std::vector<py::buffer>& nums,
                                 const Who& who, const std::vector<py::sequence>& hashes) {
    // match_batch with the tokens' own operands: strs[c][i] and nums[c][i] are token i's in column c
    auto v = as_strings(toks);
    const std::vector<Require> rq = arg_requires_of(reqs);
    std::vector<std::vector<std::string_view>> sv;
    for (const auto& col : strs) sv.emplace_back(col.begin(), col.end());
    const NumCols nc(nums, v.size());
    const HashCols hc(hashes);
    std::vector<MatchResult> rs;
    CheckStats st;
    {
      py::gil_scoped_release rel;
      rs = who.es ? s.v->MatchBatchArgsEach(views(v), *who.es, *who.w, rq, sv, nc.cols, &st, hc.cols)
                  : s.v->MatchBatchArgs(views(v), *who.e, rq, sv, nc.cols, &st, hc.cols);
    }
    py::list out(rs.size());
    for (size_t i = 0; i < rs.size(); ++i) {
      if (rs[i].ok) out[i] = py::make_tuple(py::int_(rs[i].bits), py::none());
      else out[i] = py::make_tuple(py::none(), py::str(rs[i].err));
    }
    return py::make_tuple(out, st.scanned, st.host);
  };
  auto py_match_blob_args = [=](PyValidator& s, py::bytes blob, const ArgReqList& reqs, const std::vector<py::bytes>& strs,
                                const std::vector<py::buffer>& nums, const Who& who,
                                const std::vector<py::bytes>& hashes) {
    // match_blob with the tokens' own operands: a string column is newline-separated bytes, as the tokens are;
    // so is a hash column, an empty line meaning "no value"
    char* bp = nullptr;
    Py_ssize_t bn = 0;
    if (PyBytes_AsStringAndSize(blob.ptr(), &bp, &bn) != 0) throw py::error_already_set();
    const std::vector<Require> rq = arg_requires_of(reqs);
    auto toks = split_lines(bp, (size_t)bn);
    std::vector<std::vector<std::string_view>> sv;
    for (const py::bytes& col : strs) {
      char* cp = nullptr;
      Py_ssize_t cn = 0;
      if (PyBytes_AsStringAndSize(col.ptr(), &cp, &cn) != 0) throw py::error_already_set();
      sv.push_back(split_operands(cp, (size_t)cn, toks.size()));
    }
    const NumCols nc(nums, toks.size());
    std::vector<HashColumn> hv;
    for (const py::bytes& col : hashes) {
      char* cp = nullptr;
      Py_ssize_t cn = 0;
      if (PyBytes_AsStringAndSize(col.ptr(), &cp, &cn) != 0) throw py::error_already_set();
      const std::vector<std::string_view> pieces = split_operands(cp, (size_t)cn, toks.size());
      HashColumn hcol(pieces.size());
      for (size_t i = 0; i < pieces.size(); ++i)
        if (!pieces[i].empty()) hcol[i] = pieces[i];
      hv.push_back(std::move(hcol));
    }
    py::bytes ok = fresh_bytes(toks.size()), match = fresh_bytes(4 * toks.size());
    uint8_t* const okp = (uint8_t*)bytes_mem(ok);
    uint32_t* const mp = (uint32_t*)bytes_mem(match);
    CheckStats st;
    {
      py::gil_scoped_release rel;
      if (who.es) s.v->MatchVerdictsArgsEach(toks, *who.es, *who.w, rq, sv, nc.cols, okp, mp, &st, hv);
      else s.v->MatchVerdictsArgs(toks, *who.e, rq, sv, nc.cols, okp, mp, &st, hv);
    }
    py::dict d;
    d["ok"] = ok;
    d["match"] = match;
    return py::make_tuple(d, st.scanned, st.host);
  };
  py::class_<PyValidator>(m, "Validator")
      .def(py::init([](PyKeySet* ks) {
        if (!ks) throw py::value_error("keySet must not be nil");
        auto p = std::make_unique<PyValidator>();
        p->ks = ks->ks;
        p->v = std::make_unique<Validator>(ks->ks.get());
        return p;
      }))
      .def("new_claim_set", [](PyValidator& s, const std::vector<std::string>& members, std::optional<uint32_t> seed) {
        auto p = std::make_unique<PyClaimSet>();
        p->ks = s.ks;
        py::gil_scoped_release rel;
        p->set = s.v->NewClaimSet(members, seed);
        return p;
      }, py::arg("members"), py::arg("seed") = py::none())
      .def("validate", [](PyValidator& s, py::object tok, const Expected& e) {
        std::string t = tok.cast<std::string>();
        Result r;
        {
          py::gil_scoped_release rel;
          r = s.v->Validate(t, e);
        }
        return result_py(r);
      })
      .def("validate_batch", [](PyValidator& s, py::sequence toks, const Expected& e) {
        auto v = as_strings(toks);
        Results rs;
        {
          py::gil_scoped_release rel;
          rs = s.v->ValidateBatch(views(v), e);
        }
        return results_py(rs);
      })
      .def("validate_blob", [](PyValidator& s, py::bytes blob, const Expected& e) {
        // end-to-end throughput entry: newline-separated tokens in, per-token
        // accept bytes out (claims stay on the C++ side)
        // zero-copy: the bytes object is immutable and stays referenced by the
        // caller for the duration of the call
        char* bp = nullptr;
        Py_ssize_t bn = 0;
        if (PyBytes_AsStringAndSize(blob.ptr(), &bp, &bn) != 0) throw py::error_already_set();
        std::string ok;
        {
          py::gil_scoped_release rel;
          const bool trace = std::getenv("CAPJWT_TRACE") != nullptr;
          auto t0 = std::chrono::steady_clock::now();
          auto lap = [&](const char* what) {
            if (!trace) return;
            const auto t1 = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[capjwt] blob %-12s %8.2f ms\n", what,
                         std::chrono::duration<double, std::milli>(t1 - t0).count());
            t0 = t1;
          };
          auto toks = split_lines(bp, (size_t)bn);
          lap("split");
          auto rs = s.v->ValidateBatch(toks, e);
          lap("validate");
          ok.resize(rs.size());
          for (size_t i = 0; i < rs.size(); ++i) ok[i] = rs[i].ok ? 1 : 0;
          release_results(rs);
          lap("release");
        }
        return py::bytes(ok);
      })
      .def("check_batch", [=](PyValidator& s, py::sequence toks, const Expected& e) {
        return py_check_batch(s, toks, Who{&e, nullptr, nullptr});
      })
      .def("check_batch_each", [=](PyValidator& s, py::sequence toks,
                                  const std::vector<Expected>& es, const std::vector<uint32_t>& which) {
        return py_check_batch(s, toks, Who{nullptr, &es, &which});
      })
      .def("check_blob", [=](PyValidator& s, py::bytes blob, const Expected& e) {
        return py_check_blob(s, blob, Who{&e, nullptr, nullptr});
      })
      .def("check_blob_each", [=](PyValidator& s, py::bytes blob,
                                 const std::vector<Expected>& es, py::buffer which) {
        const std::vector<uint32_t> w = which_of(which);
        return py_check_blob(s, blob, Who{nullptr, &es, &w});
      })
      .def("registered_batch", [=](PyValidator& s, py::sequence toks, const Expected& e) {
        return py_registered_batch(s, toks, Who{&e, nullptr, nullptr});
      })
      .def("registered_batch_each", [=](PyValidator& s, py::sequence toks,
                                  const std::vector<Expected>& es, const std::vector<uint32_t>& which) {
        return py_registered_batch(s, toks, Who{nullptr, &es, &which});
      })
      .def("registered_blob", [=](PyValidator& s, py::bytes blob, const Expected& e) {
        return py_registered_blob(s, blob, Who{&e, nullptr, nullptr});
      })
      .def("registered_blob_each", [=](PyValidator& s, py::bytes blob,
                                 const std::vector<Expected>& es, py::buffer which) {
        const std::vector<uint32_t> w = which_of(which);
        return py_registered_blob(s, blob, Who{nullptr, &es, &w});
      })
      .def("select_batch", [=](PyValidator& s, py::sequence toks, std::vector<std::string> names, const Expected& e) {
        return py_select_batch(s, toks, names, Who{&e, nullptr, nullptr});
      })
      .def("select_batch_each", [=](PyValidator& s, py::sequence toks, std::vector<std::string> names,
                                  const std::vector<Expected>& es, const std::vector<uint32_t>& which) {
        return py_select_batch(s, toks, names, Who{nullptr, &es, &which});
      })
      .def("select_blob", [=](PyValidator& s, py::bytes blob, std::vector<std::string> names, const Expected& e) {
        return py_select_blob(s, blob, names, Who{&e, nullptr, nullptr});
      })
      .def("select_blob_each", [=](PyValidator& s, py::bytes blob, std::vector<std::string> names,
                                 const std::vector<Expected>& es, py::buffer which) {
        const std::vector<uint32_t> w = which_of(which);
        return py_select_blob(s, blob, names, Who{nullptr, &es, &w});
      })
      .def("select_paths_batch", [=](PyValidator& s, py::sequence toks, PathList paths, const Expected& e) {
        return py_select_batch(s, toks, paths, Who{&e, nullptr, nullptr});
      })
      .def("select_paths_batch_each", [=](PyValidator& s, py::sequence toks, PathList paths,
                                        const std::vector<Expected>& es, const std::vector<uint32_t>& which) {
        return py_select_batch(s, toks, paths, Who{nullptr, &es, &which});
      })
      .def("select_paths_blob", [=](PyValidator& s, py::bytes blob, PathList paths, const Expected& e) {
        return py_select_blob(s, blob, paths, Who{&e, nullptr, nullptr});
      })
      .def("select_paths_blob_each", [=](PyValidator& s, py::bytes blob, PathList paths,
                                       const std::vector<Expected>& es, py::buffer which) {
        const std::vector<uint32_t> w = which_of(which);
        return py_select_blob(s, blob, paths, Who{nullptr, &es, &w});
      })
      .def("match_batch", [=](PyValidator& s, py::sequence toks, ReqList reqs, const Expected& e) {
        return py_match_batch(s, toks, reqs, Who{&e, nullptr, nullptr});
      })
      .def("match_batch_each", [=](PyValidator& s, py::sequence toks, ReqList reqs,
                                 const std::vector<Expected>& es, const std::vector<uint32_t>& which) {
        return py_match_batch(s, toks, reqs, Who{nullptr, &es, &which});
      })
      .def("match_blob", [=](PyValidator& s, py::bytes blob, ReqList reqs, const Expected& e) {
        return py_match_blob(s, blob, reqs, Who{&e, nullptr, nullptr});
      })
      .def("match_blob_each", [=](PyValidator& s, py::bytes blob, ReqList reqs,
                                const std::vector<Expected>& es, py::buffer which) {
        const std::vector<uint32_t> w = which_of(which);
        return py_match_blob(s, blob, reqs, Who{nullptr, &es, &w});
      })
      .def("match_batch_args", [=](PyValidator& s, py::sequence toks, ArgReqList reqs,
                                   std::vector<std::vector<std::string>> strs, std::vector<py::buffer> nums,
                                   const Expected& e, std::vector<py::sequence> hashes) {
        return py_match_batch_args(s, toks, reqs, strs, nums, Who{&e, nullptr, nullptr}, hashes);
      }, py::arg("tokens"), py::arg("requires"), py::arg("strs"), py::arg("nums"), py::arg("expected"),
         py::arg("hashes") = std::vector<py::sequence>())
      .def("match_batch_args_each", [=](PyValidator& s, py::sequence toks, ArgReqList reqs,
                                        std::vector<std::vector<std::string>> strs, std::vector<py::buffer> nums,
                                        const std::vector<Expected>& es, const std::vector<uint32_t>& which,
                                        std::vector<py::sequence> hashes) {
        return py_match_batch_args(s, toks, reqs, strs, nums, Who{nullptr, &es, &which}, hashes);
      }, py::arg("tokens"), py::arg("requires"), py::arg("strs"), py::arg("nums"), py::arg("expected"), py::arg("which"),
         py::arg("hashes") = std::vector<py::sequence>())
      .def("match_blob_args", [=](PyValidator& s, py::bytes blob, ArgReqList reqs, std::vector<py::bytes> strs,
                                  std::vector<py::buffer> nums, const Expected& e, std::vector<py::bytes> hashes) {
        return py_match_blob_args(s, blob, reqs, strs, nums, Who{&e, nullptr, nullptr}, hashes);
      }, py::arg("blob"), py::arg("requires"), py::arg("strs"), py::arg("nums"), py::arg("expected"),
         py::arg("hashes") = std::vector<py::bytes>())
      .def("match_blob_args_each", [=](PyValidator& s, py::bytes blob, ArgReqList reqs, std::vector<py::bytes> strs,
                                       std::vector<py::buffer> nums, const std::vector<Expected>& es, py::buffer which,
                                       std::vector<py::bytes> hashes) {
        const std::vector<uint32_t> w = which_of(which);
        return py_match_blob_args(s, blob, reqs, strs, nums, Who{nullptr, &es, &w}, hashes);
      }, py::arg("blob"), py::arg("requires"), py::arg("strs"), py::arg("nums"), py::arg("expected"), py::arg("which"),
         py::arg("hashes") = std::vector<py::bytes>())
      .def("_concurrent_validate", [](PyValidator& s, py::bytes blob, const Expected& e, int callers,
                                      int64_t total, int pin_cpus) {
        // Measurement helper (bench.py `single`): `callers` host threads, each
        // calling Validator::Validate once per token -- the goroutine-per-
        // request pattern of an unchanged cap caller -- over `total` tokens
        // taken round-robin from the newline-separated pool.  Returns the
        // wall time, accepts and per-call latency percentiles.
        char* bp = nullptr;
        Py_ssize_t bn = 0;
        if (PyBytes_AsStringAndSize(blob.ptr(), &bp, &bn) != 0) throw py::error_already_set();
        callers = std::max(1, callers);
        std::vector<std::vector<int64_t>> lat(callers);
        std::vector<int64_t> acc(callers, 0);
        double wall = 0;
        {
          py::gil_scoped_release rel;
          const auto toks = split_lines(bp, (size_t)bn);
          if (toks.empty()) throw std::runtime_error("empty token pool");
          std::atomic<int64_t> next{0};
          std::vector<std::thread> th;
          // pin_cpus > 0: every caller thread runs on the first pin_cpus CPUs the
          // process may use (a Go service's goroutines on GOMAXPROCS threads)
          cpu_set_t pin;
          CPU_ZERO(&pin);
          if (pin_cpus > 0) {
            cpu_set_t all;
            CPU_ZERO(&all);
            if (sched_getaffinity(0, sizeof all, &all) == 0) {
              int k = 0;
              for (int c = 0; c < CPU_SETSIZE && k < pin_cpus; ++c)
                if (CPU_ISSET(c, &all)) { CPU_SET(c, &pin); ++k; }
            }
          }
          const auto t0 = std::chrono::steady_clock::now();
          for (int c = 0; c < callers; ++c)
            th.emplace_back([&, c] {
              if (pin_cpus > 0 && CPU_COUNT(&pin) > 0) (void)sched_setaffinity(0, sizeof pin, &pin);
              lat[c].reserve((size_t)(total / callers + 16));
              while (true) {
                const int64_t i = next.fetch_add(1);
                if (i >= total) break;
                const auto a = std::chrono::steady_clock::now();
                Result r = s.v->Validate(toks[(size_t)i % toks.size()], e);
                const auto b = std::chrono::steady_clock::now();
                lat[c].push_back(std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count());
                acc[c] += r.ok;
              }
            });
          for (auto& t : th) t.join();
          wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        std::vector<int64_t> all;
        for (auto& v : lat) all.insert(all.end(), v.begin(), v.end());
        std::sort(all.begin(), all.end());
        auto pct = [&](double q) { return all.empty() ? 0.0 : (double)all[std::min(all.size() - 1, (size_t)(q * (double)all.size()))] / 1e3; };
        int64_t accepted = 0;
        for (auto a : acc) accepted += a;
        py::dict d;
        d["wall_s"] = wall;
        d["calls"] = (int64_t)all.size();
        d["accepted"] = accepted;
        d["p50_us"] = pct(0.50);
        d["p90_us"] = pct(0.90);
        d["p99_us"] = pct(0.99);
        d["p999_us"] = pct(0.999);
        d["max_us"] = all.empty() ? 0.0 : (double)all.back() / 1e3;
        return d;
      }, py::arg("blob"), py::arg("expected"), py::arg("callers"), py::arg("total"), py::arg("pin_cpus") = 0);

  // ---- go-oidc oidc.KeySet adapter (NewRemoteKeySet): payload bytes out
  struct PyRemoteKeySet {
    std::unique_ptr<RemoteKeySet> ks;
  };
  auto payload_py = [](const PayloadResult& r) {
    return py::make_tuple(r.ok ? py::object(py::bytes(r.payload)) : py::object(py::none()),
                          r.ok ? py::object(py::none()) : py::object(py::str(r.err)));
  };
  py::class_<PyRemoteKeySet>(m, "RemoteKeySet")
      .def("verify_signature", [payload_py](PyRemoteKeySet& s, py::object tok) {
        std::string t = tok.cast<std::string>();
        PayloadResult r;
        {
          py::gil_scoped_release rel;
          r = s.ks->VerifySignature(t);
        }
        return payload_py(r);
      })
      .def("verify_signature_batch", [payload_py](PyRemoteKeySet& s, py::sequence toks) {
        auto v = as_strings(toks);
        std::vector<PayloadResult> rs;
        {
          py::gil_scoped_release rel;
          rs = s.ks->VerifySignatureBatch(views(v));
        }
        py::list out;
        for (const auto& r : rs) out.append(payload_py(r));
        return out;
      })
      .def("set_coalescing", [](PyRemoteKeySet& s, int max_inflight, size_t max_batch, int64_t window_us) {
        CoalesceConfig c;
        c.max_inflight = max_inflight;
        c.max_batch = max_batch;
        c.window_us = window_us;
        s.ks->SetCoalescing(c);
      }, py::arg("max_inflight") = 2, py::arg("max_batch") = 65536, py::arg("window_us") = 0);
  m.def("new_remote_keyset", [](const std::string& url, py::object fetch, const std::vector<int>& devices) {
    auto p = std::make_unique<PyRemoteKeySet>();
    p->ks = NewRemoteKeySet(url, wrap_fetch(std::move(fetch)), devices);
    return p;
  }, py::arg("url"), py::arg("fetch"), py::arg("devices") = std::vector<int>{});

  // ---- oidc at_hash / c_hash (oidc/id_token.go:59-145) over one GPU context
  struct PyHashEngine {
    std::unique_ptr<Engine> eng;
  };
  auto hash_claims = [](PyHashEngine& s, py::sequence ids, py::sequence vals, bool code) {
    auto a = as_strings(ids), b = as_strings(vals);
    if (a.size() != b.size()) throw py::value_error("id_tokens and values differ in length");
    std::vector<HashClaimResult> rs;
    {
      py::gil_scoped_release rel;
      rs = code ? VerifyAuthorizationCodeBatch(*s.eng, views(a), views(b))
                : VerifyAccessTokenBatch(*s.eng, views(a), views(b));
    }
    py::list out;
    for (const auto& r : rs)
      out.append(py::make_tuple(r.verified, r.err.empty() ? py::object(py::none()) : py::object(py::str(r.err))));
    return out;
  };
  py::class_<PyHashEngine>(m, "HashEngine")
      .def(py::init([](const std::vector<int>& devices) {
        auto p = std::make_unique<PyHashEngine>();
        p->eng = std::make_unique<Engine>(devices);
        return p;
      }), py::arg("devices") = std::vector<int>{})
      .def("verify_access_token_batch", [hash_claims](PyHashEngine& s, py::sequence ids, py::sequence ats) {
        return hash_claims(s, ids, ats, false);
      })
      .def("verify_authorization_code_batch", [hash_claims](PyHashEngine& s, py::sequence ids, py::sequence codes) {
        return hash_claims(s, ids, codes, true);
      });
}
