// cap_jwt.cpp -- see cap_jwt.hpp.
//
// Batch flow of KeySet::verify_batch:
//   1. host threads parse every token (go-jose ParseSigned, R1-R8); compact
//      tokens take a fast path whose protected-header decode is memoised per
//      header segment (tokens signed by one issuer share it byte for byte);
//   2. each token becomes one arena entry  signing-input '.' base64url(sig):
//      canonical tokens are copied as they are, anything else is re-encoded
//      (R6), so the device always sees go-jose's computeAuthData bytes;
//   3. candidate keys per token -- static set: every key of the alg's family,
//      in order (R33); JWKS: keys whose kid matches, all keys when the token
//      has none (R34) -- become jg_tok jobs, verified in ONE jg_verify_batch;
//   4. host threads turn verdicts into (claims, error) exactly as the
//      reference's per-token loop would (first verifying key wins; the claims
//      do not depend on which key verified).
#include "cap_jwt.hpp"

#include <linux/futex.h>
#include <pthread.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <sys/resource.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <random>
#include <stdexcept>
#include <thread>
#include <unordered_map>

#include "../../../include/jg.h"
#include "hostmem.hpp"

namespace capjwt {

const char* const kSupportedAlgorithms[10] = {"RS256", "RS384", "RS512", "ES256", "ES384",
                                              "ES512", "PS256", "PS384", "PS512", "EdDSA"};

std::string SupportedSigningAlgorithm(const std::vector<std::string>& algs) {
  for (const auto& a : algs)
    if (!alg_id(a)) return "unsupported signing algorithm \"" + a + "\"";
  return "";
}

// CPUs this process may run on: the affinity mask, capped by a cgroup v2 CPU
// quota (a container's share of a large host), never a fixed number.
int available_cpus() {
  int n = (int)std::thread::hardware_concurrency();
  cpu_set_t set;
  CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char quota[32] = {0};
    long period = 0;
    if (std::fscanf(f, "%31s %ld", quota, &period) == 2 && std::strcmp(quota, "max") != 0 && period > 0) {
      const long q = std::atol(quota);
      if (q > 0) n = std::min<int>(n, (int)((q + period - 1) / period));
    }
    std::fclose(f);
  }
  return std::max(1, n);
}

int host_threads() {
  static const int n = [] {
    if (const char* e = std::getenv("CAPJWT_HOST_THREADS")) {
      const int v = std::atoi(e);
      if (v > 0) return v;
    }
    return available_cpus();
  }();
  return n;
}

namespace {

// The batch passes' worker threads, started once per process (host_threads()
// - 1 of them; the calling thread takes part too).  A ValidateBatch call runs
// ~8 parallel passes; creating 15 threads for each cost the caller a few
// hundred microseconds per pass.  A pass started from inside a pass (a nested
// call) gets threads of its own, as before.
class HostPool {
 public:
  static HostPool& get() {
    static HostPool* p = new HostPool(host_threads() - 1);   // never destroyed: threads live as long as the process
    return *p;
  }
  static bool inside() { return tl_inside_; }
  // task(i) for i in [0, nt), on the pool's threads and the caller's
  void run(size_t nt, const std::function<void(size_t)>& task) {
    Job j;
    j.fn = &task;
    j.nt = nt;
    {
      std::lock_guard<std::mutex> g(m_);
      q_.push_back(&j);
    }
    cv_.notify_all();
    size_t i;
    while ((i = take(&j)) < nt) run_one(&j, i);
    // every index finishes (a throwing task counts as finished) before j,
    // which pool threads still reference, leaves this frame
    std::unique_lock<std::mutex> lk(j.m);
    j.cv.wait(lk, [&] { return j.done == nt; });
    if (j.err) std::rethrow_exception(j.err);
  }

 private:
  struct Job {
    const std::function<void(size_t)>* fn = nullptr;
    size_t nt = 0, next = 0;        // next: under the pool's m_
    size_t done = 0;                // under m
    std::exception_ptr err;         // the first task exception, under m; rethrown by run()
    std::mutex m;
    std::condition_variable cv;
  };
  explicit HostPool(int n) {
    for (int t = 0; t < n; ++t) th_.emplace_back([this] { worker(); });
    for (auto& t : th_) t.detach();
  }
  // the next index of j (nt when none is left; the job leaves the queue with its last index)
  size_t take(Job* j) {
    std::lock_guard<std::mutex> g(m_);
    if (j->next >= j->nt) return j->nt;
    const size_t i = j->next++;
    if (j->next == j->nt) q_.erase(std::find(q_.begin(), q_.end(), j));
    return i;
  }
  static void finish(Job* j) {
    std::lock_guard<std::mutex> g(j->m);     // the owner destroys j only after taking this lock
    if (++j->done == j->nt) j->cv.notify_all();
  }
  static void run_one(Job* j, size_t i) {
    try {
      (*j->fn)(i);
    } catch (...) {
      std::lock_guard<std::mutex> g(j->m);
      if (!j->err) j->err = std::current_exception();
    }
    finish(j);
  }
  void worker() {
    pthread_setname_np(pthread_self(), "capjwt-host");
    tl_inside_ = true;
    std::unique_lock<std::mutex> lk(m_);
    while (true) {
      cv_.wait(lk, [&] { return !q_.empty(); });
      Job* j = q_.front();
      const size_t i = j->next++;
      if (j->next == j->nt) q_.pop_front();
      lk.unlock();
      run_one(j, i);
      lk.lock();
    }
  }
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<Job*> q_;
  std::vector<std::thread> th_;
  static thread_local bool tl_inside_;
};
thread_local bool HostPool::tl_inside_ = false;

// fn(i) for i in [0, nt) on nt threads (the pool's, or new ones for a nested call)
template <class F>
void run_parallel(size_t nt, F&& fn) {
  if (!HostPool::inside() && nt <= (size_t)host_threads()) {
    const std::function<void(size_t)> task = [&fn](size_t i) { fn(i); };
    HostPool::get().run(nt, task);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(nt);
  for (size_t t = 0; t < nt; ++t) th.emplace_back([&fn, t] { fn(t); });
  for (auto& t : th) t.join();
}

template <class F>
void parallel_for(size_t n, int threads, F&& fn) {
  // fn(begin, end): contiguous chunks; small batches stay on the caller's thread
  const size_t min_chunk = 512;
  const size_t nt = std::min<size_t>((size_t)std::max(1, threads), (n + min_chunk - 1) / min_chunk);
  if (nt <= 1) {
    if (n) fn((size_t)0, n);
    return;
  }
  run_parallel(nt, [&](size_t t) { fn(n * t / nt, n * (t + 1) / nt); });
}

// A fixed cut of [0, n) into per-thread ranges, so that several passes over a
// batch (count, prefix, fill) see the same ranges and keep running offsets per
// range instead of one serial prefix sum over every token.
struct Chunks {
  std::vector<size_t> b;        // range c = [b[c], b[c+1])
  size_t count() const { return b.size() - 1; }
};
Chunks make_chunks(size_t n, int threads) {
  const size_t min_chunk = 512;
  const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), (n + min_chunk - 1) / min_chunk));
  Chunks c;
  c.b.resize(nt + 1);
  for (size_t t = 0; t <= nt; ++t) c.b[t] = n * t / nt;
  return c;
}
template <class F>
void run_chunks(const Chunks& c, F&& fn) {
  // fn(chunk, begin, end)
  if (c.count() == 1) {
    fn((size_t)0, c.b[0], c.b[1]);
    return;
  }
  run_parallel(c.count(), [&](size_t t) { fn(t, c.b[t], c.b[t + 1]); });
}

}  // namespace

void* batch_block_alloc(size_t bytes, size_t* cap) {
  if (bytes >= (size_t(1) << 20)) return hostmem::big_get(bytes, cap);
  *cap = bytes;
  return ::operator new(bytes);
}

void batch_block_free(void* p, size_t cap) {
  if (!p) return;
  if (cap >= (size_t(1) << 20)) hostmem::big_put(p, cap);
  else ::operator delete(p);
}

void SetHostMemoryRetention(size_t bytes) { hostmem::set_retention_cap(bytes); }
void TrimHostMemory() { hostmem::trim(); }
size_t HostMemoryRetained() { return hostmem::retained(); }

void batch_parallel(size_t n, int threads, const std::function<void(size_t, size_t)>& fn) {
  parallel_for(n, threads, fn);
}

namespace {

int64_t wall_now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::system_clock::now().time_since_epoch())
      .count();
}

// ---------------------------------------------------------------- per-token parse
struct HdrInfo {                 // one decoded protected-header segment (compact form)
  bool b64_ok = false;
  std::string b64_err;
  bool ok = false;               // JSON + sanitize
  std::string err;
  Signature sig;                 // protected_raw / protected_hdr / alg / kid
  bool seg_canonical = false;
  bool verifiable = false;       // crit understood, non-empty protected bytes
  bool needs_b64 = true;
  int alg = 0;
};

std::shared_ptr<const HdrInfo> make_hdr(std::string_view seg) {
  auto h = std::make_shared<HdrInfo>();
  h->b64_ok = b64url_decode(seg, &h->sig.protected_raw, &h->b64_err);
  if (!h->b64_ok) return h;
  // parse the header exactly as parse_signed does, on a minimal token
  JWS j;
  std::string tok = b64url_encode(h->sig.protected_raw) + "..";
  if (!parse_signed(tok, &j, &h->err)) return h;
  h->ok = true;
  h->sig = j.sigs[0];
  h->seg_canonical = b64url_canonical(seg);
  std::string si;
  h->verifiable = signing_input(j, &si);       // payload "" -> crit / protected checks only
  if (const json::Value* b = h->sig.protected_hdr.get("b64"); b && b->kind == json::Value::Bool) h->needs_b64 = b->b;
  h->alg = alg_id(h->sig.alg);
  return h;
}

struct HdrCache {
  // a few recent segments checked by plain compare first (a key set's tokens
  // cycle through a handful of headers), then the map
  static constexpr int NRECENT = 8;
  std::string recent_key[NRECENT];
  std::shared_ptr<const HdrInfo> recent_val[NRECENT];
  int nrecent = 0, next = 0;
  // the cache lives as long as its pool thread and its segments come from
  // callers: it is bounded by bytes, and a segment above kMaxSeg (far above
  // any issuer's header) is decoded for this token only
  static constexpr size_t kMaxSeg = 1024, kMaxBytes = 1 << 20;
  std::unordered_map<std::string, std::shared_ptr<const HdrInfo>> m;
  size_t bytes = 0;
  std::shared_ptr<const HdrInfo> uncached;
  const std::shared_ptr<const HdrInfo>& get(std::string_view seg) {
    for (int i = 0; i < nrecent; ++i)
      if (recent_key[i] == seg) return recent_val[i];
    if (seg.size() > kMaxSeg) {
      uncached = make_hdr(seg);
      return uncached;
    }
    auto it = m.find(std::string(seg));
    if (it == m.end()) {
      if (bytes + seg.size() > kMaxBytes) {
        m.clear();
        bytes = 0;
      }
      it = m.emplace(std::string(seg), make_hdr(seg)).first;
      bytes += seg.size() + 64;
    }
    const int slot = next;
    next = (next + 1) % NRECENT;
    if (nrecent < NRECENT) ++nrecent;
    recent_key[slot].assign(seg);
    recent_val[slot] = it->second;
    return recent_val[slot];
  }
};

// decoded length of a base64url segment with no '=' (Go RawURLEncoding)
inline size_t b64_decoded_len(size_t n) { return n / 4 * 3 + (n % 4 == 2 ? 1 : n % 4 == 3 ? 2 : 0); }

struct PhaseTimer {            // CAPJWT_TRACE=1: per-phase wall times (and page faults) on stderr
  bool on;
  std::chrono::steady_clock::time_point t0;
  long flt0 = 0;
  const char* what;
  static long minflt() {
    rusage ru;
    getrusage(RUSAGE_SELF, &ru);
    return ru.ru_minflt;
  }
  explicit PhaseTimer(const char* w) : on(std::getenv("CAPJWT_TRACE") != nullptr), t0(std::chrono::steady_clock::now()), what(w) {
    if (on) flt0 = minflt();
  }
  void lap(const char* phase) {
    if (!on) return;
    const auto t1 = std::chrono::steady_clock::now();
    const long f = minflt();
    std::fprintf(stderr, "[capjwt] %s %-12s %7ld flt %8.2f ms\n", what, phase, f - flt0,
                 std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
    flt0 = f;
  }
};

// Array whose elements are constructed and destroyed by all host threads
// (a 1M-token batch's per-token records are ~200 MB of strings: serial
// construction/destruction cost more than the parse itself).
template <class T>
struct ParArray {
  T* p = nullptr;
  size_t n = 0, cap = 0;
  int threads = 1;
  ParArray() = default;
  ParArray(const ParArray&) = delete;
  ParArray& operator=(const ParArray&) = delete;
  void init(size_t count, int th);
  void release();
  ~ParArray() { release(); }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
  size_t size() const { return n; }
};

// Decoded payloads of one parse range, in pooled hostmem blocks (one return
// per block instead of one free per token; no page faults in steady state)
struct ByteArena {
  std::vector<void*> blocks;                      // hostmem::kBlock each
  std::vector<std::unique_ptr<char[]>> big;       // payloads larger than a block
  char* cur = nullptr;
  size_t left = 0;
  ByteArena() = default;
  ByteArena(ByteArena&& o) noexcept
      : blocks(std::move(o.blocks)), big(std::move(o.big)), cur(o.cur), left(o.left), last_big(o.last_big) {
    o.cur = nullptr;
    o.left = 0;
  }
  ByteArena(const ByteArena&) = delete;
  ByteArena& operator=(const ByteArena&) = delete;
  ~ByteArena() {
    for (void* b : blocks) hostmem::block_put(b);
  }
  bool last_big = false;
  char* alloc(size_t n) {
    last_big = n > hostmem::kBlock / 2;
    if (last_big) {
      big.emplace_back(new char[n]);
      return big.back().get();
    }
    if (n > left) {
      blocks.push_back(hostmem::block_get());
      cur = static_cast<char*>(blocks.back());
      left = hostmem::kBlock;
    }
    char* r = cur;
    cur += n;
    left -= n;
    return r;
  }
  void give_back(size_t n) {     // the unused tail of the last alloc (a block's, not a big one's)
    if (last_big) return;
    cur -= n;
    left += n;
  }
};

struct GeneralParse {            // storage of a token that took jose.ParseSigned's general path
  std::string alg, kid, payload;
};

struct Tok {
  // ParseSigned outcome (validateSigningAlgorithm's inputs)
  bool parsed = false;
  bool verifiable = false;     // DetachedVerify gets as far as verifyPayload
  int alg = 0;
  uint32_t nsigs = 0;
  size_t sig0_len = 0;
  std::string parse_err;
  std::string_view alg_name, kid, payload;     // into hdr / gen / the batch's ByteArena
  std::shared_ptr<const HdrInfo> hdr;           // compact path: the shared header decode
  std::unique_ptr<GeneralParse> gen;
  // arena entry: literal token span, or owned bytes
  const char* lit = nullptr;
  size_t lit_len = 0;
  std::string owned;
  uint32_t si_len = 0, sig_b64_len = 0;
  uint32_t ncand = 0;          // candidate keys (jobs) in the current GPU batch
  uint64_t job0 = 0;           // first job of this token in that batch
  size_t entry_len() const { return lit ? lit_len : owned.size(); }
  TokenView view() const { return TokenView{parsed, parse_err, nsigs, sig0_len, alg_name}; }
};

template <class T>
void ParArray<T>::init(size_t count, int th) {
  release();
  threads = th;
  p = static_cast<T*>(batch_block_alloc(sizeof(T) * (count ? count : 1), &cap));
  n = count;
  parallel_for(n, threads, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) new (p + i) T();
  });
}

template <class T>
void ParArray<T>::release() {
  if (!p) return;
  parallel_for(n, threads, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) p[i].~T();
  });
  batch_block_free(p, cap);
  p = nullptr;
  n = 0;
}

void parse_one(std::string_view token, HdrCache& cache, ByteArena& pay, Tok* t) {
  // compact fast path: no whitespace / non-ASCII, exactly three segments
  if (!token.empty() && token[0] != '{' && !has_go_space_or_nonascii(token)) {
    const size_t d1 = token.find('.');
    const size_t d2 = d1 == std::string_view::npos ? d1 : token.find('.', d1 + 1);
    if (d1 == std::string_view::npos || d2 == std::string_view::npos ||
        token.find('.', d2 + 1) != std::string_view::npos) {
      t->parse_err = "square/go-jose: compact JWS format must have three parts";
      return;
    }
    const std::string_view hs = token.substr(0, d1), ps = token.substr(d1 + 1, d2 - d1 - 1),
                           ss = token.substr(d2 + 1);
    const std::shared_ptr<const HdrInfo>& h = cache.get(hs);
    // parseSignedCompact order: protected, payload, signature decodes, then sanitize
    if (!h->b64_ok) { t->parse_err = h->b64_err; return; }
    bool pay_canon = false;
    {
      const size_t cap = ps.size() / 4 * 3 + 2;
      char* dst = pay.alloc(cap);
      const long len = b64url_decode_fast(ps, dst, &pay_canon);
      if (len >= 0) {
        pay.give_back(cap - (size_t)len);
        t->payload = std::string_view(dst, (size_t)len);
      } else {                 // '=', CR/LF or an illegal byte: Go's skipping and error text
        pay.give_back(cap);
        t->gen = std::make_unique<GeneralParse>();
        if (!b64url_decode(ps, &t->gen->payload, &t->parse_err)) return;
        t->payload = t->gen->payload;
        pay_canon = false;
      }
    }
    // the signature bytes themselves are only needed when the segment is not
    // canonical (the device decodes canonical base64url itself)
    const bool sig_canon = b64url_canonical(ss);
    std::string sig;
    size_t siglen;
    if (sig_canon) {
      siglen = b64_decoded_len(ss.size());
    } else {
      if (!b64url_decode(ss, &sig, &t->parse_err)) return;
      siglen = sig.size();
    }
    if (!h->ok) { t->parse_err = h->err; return; }
    t->parsed = true;
    t->nsigs = 1;
    t->sig0_len = siglen;
    t->hdr = h;
    t->alg_name = h->sig.alg;
    t->kid = h->sig.kid;
    t->alg = h->alg;
    t->verifiable = h->verifiable && t->alg != 0;
    if (!t->verifiable) return;
    if (h->seg_canonical && h->needs_b64 && pay_canon && sig_canon) {
      t->lit = token.data();
      t->lit_len = token.size();
      t->si_len = (uint32_t)d2;
      t->sig_b64_len = (uint32_t)ss.size();
      return;
    }
    JWS j;
    j.payload = std::string(t->payload);
    j.sigs.push_back(h->sig);
    std::string si;
    signing_input(j, &si);
    t->si_len = (uint32_t)si.size();
    t->owned = std::move(si);
    t->owned.push_back('.');
    const std::string sb = sig_canon ? std::string(ss) : b64url_encode(sig);
    t->sig_b64_len = (uint32_t)sb.size();
    t->owned += sb;
    return;
  }
  // general path: jose.ParseSigned
  JWS j;
  if (!parse_signed(token, &j, &t->parse_err)) return;
  t->parsed = true;
  t->nsigs = (uint32_t)j.sigs.size();
  t->sig0_len = j.sigs.empty() ? 0 : j.sigs[0].signature.size();
  t->gen = std::make_unique<GeneralParse>();
  t->gen->alg = j.sigs.empty() ? "" : j.sigs[0].alg;
  t->gen->kid = j.sigs.empty() ? "" : j.sigs[0].kid;      // go-oidc: the first signature's kid
  t->gen->payload = j.payload;
  t->alg_name = t->gen->alg;
  t->kid = t->gen->kid;
  t->payload = t->gen->payload;
  std::string si;
  if (!signing_input(j, &si)) return;
  t->alg = alg_id(j.sigs[0].alg);
  t->verifiable = t->alg != 0;
  if (!t->verifiable) return;
  t->si_len = (uint32_t)si.size();
  t->owned = std::move(si);
  t->owned.push_back('.');
  const std::string sb = b64url_encode(j.sigs[0].signature);
  t->sig_b64_len = (uint32_t)sb.size();
  t->owned += sb;
}

// json.Unmarshal(payload, &map[string]interface{})  [R33, R35, R40]
bool claims_map(std::string_view payload, json::Value* out, std::string* err) {
  if (!json::parse(payload, out, err)) return false;
  if (out->is_null()) return true;
  if (out->kind != json::Value::Object) {
    static const char* names[] = {"null", "bool", "number", "string", "array", "object"};
    *err = std::string("json: cannot unmarshal ") + names[out->kind] + " into Go value of type map[string]interface {}";
    return false;
  }
  if (json::has_range_error(*out)) {
    *err = "json: cannot unmarshal number into Go value of type float64";
    return false;
  }
  return true;
}

jg_key to_jg(const PublicKey& k) {
  jg_key o{};
  switch (k.kind) {
    case PublicKey::RSA:
      o.kind = JG_KEY_RSA;
      o.n = (const uint8_t*)k.n.data();
      o.n_len = (int32_t)k.n.size();
      o.e = k.e;
      break;
    case PublicKey::EC:
      o.kind = JG_KEY_EC;
      o.curve = k.curve;
      o.x = (const uint8_t*)k.x.data();
      o.y = (const uint8_t*)k.y.data();
      o.coord_len = (int32_t)k.x.size();
      break;
    case PublicKey::Ed25519:
      o.kind = JG_KEY_ED25519;
      o.x = (const uint8_t*)k.x.data();
      o.coord_len = (int32_t)k.x.size();
      break;
    default:
      o.kind = 0;         // HMAC secret / private key / nothing: verifies no token on this path
  }
  return o;
}

int key_family(const PublicKey& k) {
  switch (k.kind) {
    case PublicKey::RSA: return JG_KEY_RSA;
    case PublicKey::EC: return JG_KEY_EC;
    case PublicKey::Ed25519: return k.x.size() == 32 ? JG_KEY_ED25519 : 0;
    default: return 0;
  }
}

// The GPU half shared by both key sets: parse, pack, verify.  `cand(t, push)`
// pushes the key indices to try for token t.  `keys_lock` (may be null) is the
// caller's lock on its key list, held from the first cand() call until the
// jobs are queued on the device and released there (jg_submit captures the
// device key table that the candidate indices refer to).
}  // namespace

// A batch after parse and device verification, before claims (KeySet::verify_raw)
struct Verified {
  ParArray<Tok> toks;
  std::vector<ByteArena> payloads;   // one per parse range
  std::vector<uint8_t> any;          // some candidate key verified
  // degraded path (SURVEY §5 failure row): when the device call fails (a HIP
  // error, a lost device) the tokens it carried are marked here and get
  // dev_err as their error -- no CPU verification, no exception out of the
  // batch; dev_seen = the engine's error count then (for Engine::recover)
  std::vector<uint8_t> failed;
  std::string dev_err;
  uint64_t dev_seen = 0;
  bool dev_failed = false;
  std::string miss_err;              // JWKS: the error of a parsed token no key verified
  // during the Overlap call only: the pinned arena the device verifies from
  // and its jobs (token t's entry starts at jobs[t.job0].off) -- CheckBatch
  // scans the payload segments in place there
  const uint8_t* arena = nullptr;
  size_t arena_len = 0;
  const jg_tok* jobs = nullptr;
};

namespace {

template <class Cand>
void gpu_verify(Engine& eng, const std::vector<std::string_view>& tokens, Verified* V, Cand&& cand,
                const std::vector<size_t>* subset = nullptr, std::shared_lock<std::shared_mutex>* keys_lock = nullptr,
                const KeySet::Overlap* overlap = nullptr) {
  const size_t n = subset ? subset->size() : tokens.size();
  auto tok_index = [&](size_t i) { return subset ? (*subset)[i] : i; };
  auto release_keys = [&] {
    if (keys_lock && keys_lock->owns_lock()) keys_lock->unlock();
  };
  PhaseTimer pt("verify");
  const Chunks ch = make_chunks(n, eng.threads());
  if (!subset) {
    V->toks.init(tokens.size(), eng.threads());
    V->any.assign(tokens.size(), 0);
    V->failed.assign(tokens.size(), 0);
    V->payloads.resize(ch.count());
    run_chunks(ch, [&](size_t c, size_t lo, size_t hi) {
      // per thread and kept across batches: a coalesced single-token batch
      // finds its issuer's header decoded already (make_hdr is a pure function
      // of the segment; entries are immutable and shared)
      thread_local HdrCache cache;
      for (size_t i = lo; i < hi; ++i) parse_one(tokens[i], cache, V->payloads[c], &V->toks[i]);
    });
    pt.lap("parse");
  }
  // pass 1: candidate keys per token, arena bytes and jobs per range
  std::vector<uint64_t> rbytes(ch.count() + 1, 0), rjobs(ch.count() + 1, 0);
  run_chunks(ch, [&](size_t c, size_t lo, size_t hi) {
    std::vector<uint16_t> ks;
    uint64_t bytes = 0, jobs = 0;
    for (size_t i = lo; i < hi; ++i) {
      Tok& t = V->toks[tok_index(i)];
      ks.clear();
      if (t.verifiable) cand(t, ks);
      t.ncand = (uint32_t)ks.size();
      if (t.ncand) bytes += t.entry_len();
      jobs += t.ncand;
    }
    rbytes[c + 1] = bytes;
    rjobs[c + 1] = jobs;
  });
  for (size_t c = 0; c < ch.count(); ++c) {
    rbytes[c + 1] += rbytes[c];
    rjobs[c + 1] += rjobs[c];
  }
  const size_t total_jobs = rjobs[ch.count()];
  pt.lap("plan");
  if (total_jobs == 0) {
    release_keys();
    return;
  }
  const uint64_t arena_len = rbytes[ch.count()];
  Engine::Pinned arena = eng.pinned(arena_len);
  std::unique_ptr<jg_tok[]> jobs(new jg_tok[total_jobs]);      // filled below, not zeroed first
  std::unique_ptr<uint8_t[]> verdict(new uint8_t[total_jobs]);
  // pass 2: pack the arena and the jobs, each range from its own offsets
  run_chunks(ch, [&](size_t c, size_t lo, size_t hi) {
    std::vector<uint16_t> ks;
    uint64_t off = rbytes[c], jn = rjobs[c];
    for (size_t i = lo; i < hi; ++i) {
      Tok& t = V->toks[tok_index(i)];
      if (!t.ncand) continue;
      const size_t len = t.entry_len();
      std::memcpy(arena.get() + off, t.lit ? t.lit : t.owned.data(), len);
      ks.clear();
      cand(t, ks);
      t.job0 = jn;
      for (size_t k = 0; k < ks.size(); ++k) {
        jg_tok& j = jobs[jn + k];
        j.off = off;
        j.sig_in_len = t.si_len;
        j.sig_rel_off = t.si_len + 1;
        j.sig_b64_len = t.sig_b64_len;
        j.key_idx = ks[k];
        j.alg = (uint8_t)t.alg;
        j.flags = 0;
      }
      off += len;
      jn += ks.size();
    }
  });
  pt.lap("pack");
  try {
    eng.verify(arena.get(), arena_len, jobs.get(), total_jobs, verdict.get(), [&] {
      release_keys();
      if (overlap) {
        V->arena = arena.get();
        V->arena_len = arena_len;
        V->jobs = jobs.get();
        try {
          (*overlap)(*V);
        } catch (...) {
          V->arena = nullptr;
          V->jobs = nullptr;
          throw;
        }
        V->arena = nullptr;
        V->jobs = nullptr;
        pt.lap("overlap");
      }
    });
  } catch (const DeviceError& e) {
    release_keys();
    V->dev_err = std::string("capjwt: signature verification unavailable: ") + e.what();
    V->dev_seen = eng.errors();
    V->dev_failed = true;
    run_chunks(ch, [&](size_t, size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i)
        if (V->toks[tok_index(i)].ncand) V->failed[tok_index(i)] = 1;
    });
    return;
  }
  pt.lap("gpu");
  run_chunks(ch, [&](size_t, size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      const size_t ti = tok_index(i);
      const Tok& t = V->toks[ti];
      for (uint32_t k = 0; k < t.ncand; ++k)
        if (verdict[t.job0 + k] == JG_ACCEPT) V->any[ti] = 1;
    }
  });
  pt.lap("verdicts");
}

// After a batch whose device call failed: recreate the context so that the
// next call verifies again (Engine::recover; no key refetch)
void recover_after(Engine& eng, const Verified& V) {
  if (V.dev_failed) (void)eng.recover(V.dev_seen);
}

// ---------------------------------------------------------------- static key set
class StaticKeySet final : public KeySet {
 public:
  StaticKeySet(const std::vector<PublicKey>& keys, const std::vector<int>& devices) : keys_(keys), eng_(devices) {
    eng_.load(keys_);
    for (const auto& k : keys_) fam_.push_back(key_family(k));
  }
  void WaitTables() override { eng_.wait_tables(); }
  std::string DeviceStatus() override { return eng_.status(); }
  int DeviceRecoveries() override { return eng_.recoveries(); }
  int DebugFailVerify(int n) override { return eng_.debug_fail_verify(n); }
  Engine& engine() override { return eng_; }
  // The key list never changes: no lock; concurrent calls pipeline on the device.
  std::shared_ptr<Verified> verify_raw(const std::vector<std::string_view>& tokens,
                                       const Overlap* overlap = nullptr) override {
    auto V = std::make_shared<Verified>();
    gpu_verify(eng_, tokens, V.get(), [&](const Tok& t, std::vector<uint16_t>& out) {
      // staticKeySet: every key in order (jwt/keyset.go:162-168); a key of
      // another family fails newVerifier/verifyPayload without arithmetic (R10)
      const int fam = alg_key_kind(t.alg);
      for (size_t k = 0; k < keys_.size(); ++k)
        if (fam_[k] == fam) out.push_back((uint16_t)k);
    }, nullptr, nullptr, overlap);
    recover_after(eng_, *V);
    return V;
  }
  void finish(const Verified& V, size_t i, Result& r) override {
    const Tok& t = V.toks[i];
    if (!t.parsed) {
      r.err = t.parse_err;                                           // jwt.ParseSigned error
    } else if (V.failed[i]) {
      r.err = V.dev_err;
    } else {
      std::string jerr;
      // parsedJWT.Claims(key, &allClaims): verify, then unmarshal; a JSON
      // error moves on to the next key, so it ends as "no known key"
      if (V.any[i] && claims_map(t.payload, &r.claims, &jerr)) {
        r.ok = true;
      } else {
        r.claims = json::Value();
        r.err = "no known key successfully validated the token signature";
      }
    }
  }
  void finish_pre(const Verified& V, size_t i, Result& r, bool json_ok) override {
    if (V.failed[i]) {
      r.claims = json::Value();
      r.err = V.dev_err;
    } else if (V.any[i] && json_ok) {
      r.err.clear();
      r.ok = true;
    } else {
      r.claims = json::Value();
      r.err = "no known key successfully validated the token signature";
    }
  }
  const char* trace_name() const override { return "static"; }

 private:
  std::vector<PublicKey> keys_;
  std::vector<int> fam_;
  Engine eng_;
};

// ---------------------------------------------------------------- JWKS key set (go-oidc v2.2.1 remoteKeySet)
bool ca_pem_ok(const std::string& pem) {
  // x509.CertPool.AppendCertsFromPEM: true iff at least one CERTIFICATE block parses
  std::string_view rest = pem;
  bool any = false;
  while (true) {
    const size_t b = rest.find("-----BEGIN CERTIFICATE-----");
    if (b == std::string_view::npos) break;
    const size_t e = rest.find("-----END CERTIFICATE-----", b);
    if (e == std::string_view::npos) break;
    const std::string_view block = rest.substr(b, e + 25 - b);
    std::string body;
    const size_t hs = block.find('\n');
    for (char c : block.substr(hs == std::string_view::npos ? 0 : hs, block.size() - 25 - (hs == std::string_view::npos ? 0 : hs)))
      if (c != ' ' && c != '\t' && c != '\r' && c != '\n') body.push_back(c);
    std::string der, err;
    PublicKey pk;
    if (b64std_decode(body, &der) && parse_certificate_public_key(der, &pk, &err)) any = true;
    rest = rest.substr(e + 25);
  }
  return any;
}

class JSONWebKeySet final : public KeySet {
 public:
  JSONWebKeySet(std::string url, std::string ca, Fetcher f, const std::vector<int>& devices)
      : url_(std::move(url)), ca_(std::move(ca)), fetch_(std::move(f)), eng_(devices) {}

  void WaitTables() override { eng_.wait_tables(); }
  std::string DeviceStatus() override { return eng_.status(); }
  int DeviceRecoveries() override { return eng_.recoveries(); }
  int DebugFailVerify(int n) override { return eng_.debug_fail_verify(n); }
  Engine& engine() override { return eng_; }
  std::shared_ptr<Verified> verify_raw(const std::vector<std::string_view>& tokens,
                                       const Overlap* overlap = nullptr) override {
    auto V = std::make_shared<Verified>();
    remote_verify(tokens, V.get(), &V->miss_err, overlap);
    return V;
  }
  void finish(const Verified& V, size_t i, Result& r) override {
    const Tok& t = V.toks[i];
    if (!t.parsed) {
      r.err = "oidc: malformed jwt: " + t.parse_err;
    } else if (V.failed[i]) {
      r.err = V.dev_err;
    } else if (!V.any[i]) {
      r.err = V.miss_err;
    } else {
      std::string jerr;       // jsonWebKeySet.VerifySignature: json.Unmarshal(payload)
      if (claims_map(t.payload, &r.claims, &jerr)) r.ok = true;
      else { r.claims = json::Value(); r.err = jerr; }
    }
  }
  void finish_pre(const Verified& V, size_t i, Result& r, bool json_ok) override {
    if (V.failed[i]) {
      r.claims = json::Value();
      r.err = V.dev_err;
    } else if (!V.any[i]) {
      r.claims = json::Value();
      r.err = V.miss_err;
    } else if (json_ok) {
      r.err.clear();
      r.ok = true;
    } else {
      r.claims = json::Value();                  // r.err: the JSON error
    }
  }
  const char* trace_name() const override { return "jwks"; }

  // go-oidc remoteKeySet.VerifySignature itself: token i's verified payload bytes
  static PayloadResult payload_result(const Verified& V, size_t i) {
    PayloadResult r;
    const Tok& t = V.toks[i];
    if (!t.parsed) r.err = "oidc: malformed jwt: " + t.parse_err;
    else if (V.failed[i]) r.err = V.dev_err;
    else if (!V.any[i]) r.err = V.miss_err;
    else { r.ok = true; r.payload = std::string(t.payload); }
    return r;
  }
  std::vector<PayloadResult> verify_payload_batch(const std::vector<std::string_view>& tokens) {
    auto V = verify_raw(tokens);
    std::vector<PayloadResult> res(tokens.size());
    parallel_for(tokens.size(), eng_.threads(), [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) res[i] = payload_result(*V, i);
    });
    return res;
  }

 private:
  // remoteKeySet.verify over a batch: kid-filtered keys from the cache, then
  // (for the tokens that missed) one refresh if the cache has expired and a
  // retry.  *miss_err = the error every unverified, parsed token gets.
  //
  // Concurrency: the key list (keys_, fam_) is read under a shared lock from
  // candidate selection until the jobs are queued (gpu_verify), and replaced
  // under the exclusive lock by refresh() -- a refresh never waits for a device
  // call, and no call's jobs can name a key of a list the device does not hold.
  // Refreshes are serialised.  As in go-oidc, the expiry a call tests is the
  // one it read with the cached keys; a call that needs remote keys while
  // another call's refresh completed since its read takes that refresh's
  // outcome (go-oidc's keysFromRemote shares an in-flight request the same way).
  void remote_verify(const std::vector<std::string_view>& tokens, Verified* V, std::string* miss_err,
                     const Overlap* overlap) {
    auto cand = [&](const Tok& t, std::vector<uint16_t>& out) {
      // remoteKeySet.verify: keyID == "" || key.KeyID == keyID   [R31, R34]
      const int fam = alg_key_kind(t.alg);
      for (size_t k = 0; k < keys_.size(); ++k)
        if ((t.kid.empty() || keys_[k].kid == t.kid) && fam_[k] == fam) out.push_back((uint16_t)k);
    };
    uint64_t seen_refreshes;
    int64_t seen_expiry;
    bool seen_have;
    {
      std::shared_lock<std::shared_mutex> lk(keys_mu_);
      seen_refreshes = refreshes_;
      seen_expiry = expiry_ns_;
      seen_have = have_keys_;
      if (have_keys_) gpu_verify(eng_, tokens, V, cand, nullptr, &lk, overlap);
      else gpu_verify(eng_, tokens, V, [](const Tok&, std::vector<uint16_t>&) {}, nullptr, &lk, overlap);
    }
    recover_after(eng_, *V);
    // tokens that parsed but did not verify: refresh once if the cache has
    // expired (now + keysExpiryDelta(30s) after expiry), then retry them.  A
    // token whose device call failed is no miss: it keeps the device error and
    // triggers no refetch
    std::vector<size_t> miss;
    for (size_t i = 0; i < tokens.size(); ++i)
      if (V->toks[i].parsed && !V->any[i] && !V->failed[i]) miss.push_back(i);
    std::string fetch_err;
    bool refreshed = false;
    if (!miss.empty() && (!seen_have || wall_now_ns() + 30 * kSecond > seen_expiry)) {
      refreshed = true;
      std::lock_guard<std::mutex> rg(refresh_mu_);
      bool ok;
      if (refreshes_ != seen_refreshes) {            // joined a refresh that completed meanwhile
        ok = last_refresh_ok_;
        fetch_err = last_fetch_err_;
      } else {
        ok = refresh(&fetch_err);
        std::unique_lock<std::shared_mutex> lk(keys_mu_);
        ++refreshes_;
        last_refresh_ok_ = ok;
        last_fetch_err_ = fetch_err;
      }
      if (ok) {
        std::shared_lock<std::shared_mutex> lk(keys_mu_);
        gpu_verify(eng_, tokens, V, cand, &miss, &lk);
      }
    }
    recover_after(eng_, *V);
    *miss_err = refreshed && !fetch_err.empty() ? "fetching keys " + fetch_err : "failed to verify id token signature";
  }

  // go-oidc updateKeys; the caller holds refresh_mu_
  bool refresh(std::string* err) {
    FetchResponse resp;
    try {
      resp = fetch_(url_, ca_);
    } catch (const std::exception& e) {
      *err = std::string("oidc: get keys failed ") + e.what();
      return false;
    }
    if (resp.status != 200) {
      *err = "oidc: get keys failed: " + resp.status_text + " " + resp.body;
      return false;
    }
    const int64_t expiry = wall_now_ns() + (resp.max_age_s > 0 ? resp.max_age_s * kSecond : 0);
    // an unchanged document (the usual refresh-on-miss answer for a tampered
    // token): the cached keys stand as they are -- no decode, no device work
    {
      std::unique_lock<std::shared_mutex> lk(keys_mu_);
      if (have_keys_ && resp.body == body_) {
        expiry_ns_ = expiry;
        return true;
      }
    }
    std::vector<JSONWebKey> keys;
    std::string derr;
    if (!jwks_decode(resp.body, &keys, &derr)) {
      *err = "oidc: failed to decode keys: " + derr + " " + resp.body;
      return false;
    }
    if (keys.size() > 65535) { *err = "oidc: too many keys"; return false; }
    // the new key list is committed only once the device table holds it: a
    // failed staging keeps the previous cache, as go-oidc keeps its cached
    // keys when updateKeys fails
    std::vector<PublicKey> pk;
    std::vector<int> fam;
    for (const auto& k : keys) {
      pk.push_back(k.key);
      fam.push_back(key_family(k.key));
    }
    std::unique_lock<std::shared_mutex> lk(keys_mu_);
    try {
      eng_.load(pk);
    } catch (const std::exception& e) {
      *err = std::string("oidc: failed to stage keys: ") + e.what();
      return false;
    }
    fam_ = std::move(fam);
    keys_ = std::move(keys);
    body_ = std::move(resp.body);
    have_keys_ = true;
    expiry_ns_ = expiry;
    return true;
  }

  std::string url_, ca_;
  Fetcher fetch_;
  Engine eng_;
  std::shared_mutex keys_mu_;     // keys_, fam_, body_, have_keys_, expiry_ns_, refreshes_, last_*
  std::mutex refresh_mu_;         // one refresh at a time
  std::vector<JSONWebKey> keys_;
  std::vector<int> fam_;
  std::string body_;              // the JWKS document keys_ came from
  bool have_keys_ = false;
  int64_t expiry_ns_ = 0;
  uint64_t refreshes_ = 0;        // refresh attempts completed
  bool last_refresh_ok_ = false;  // ... and the last one's outcome
  std::string last_fetch_err_;
};

// ---------------------------------------------------------------- Go time arithmetic
constexpr int64_t kUnixToInternal = 62135596800LL;   // time.unixToInternal
struct GoTime {
  int64_t sec;     // seconds since year 1 (Time.ext without monotonic)
  int64_t nsec;    // [0, 1e9)
};
GoTime go_now(int64_t unix_ns) {
  int64_t s = unix_ns / kSecond, ns = unix_ns % kSecond;
  if (ns < 0) { ns += kSecond; --s; }
  return {s + kUnixToInternal, ns};
}
GoTime go_add(GoTime t, int64_t d) {                  // Time.Add
  int64_t dsec = d / kSecond;
  int64_t nsec = t.nsec + d % kSecond;
  if (nsec >= kSecond) { ++dsec; nsec -= kSecond; }
  else if (nsec < 0) { --dsec; nsec += kSecond; }
  const int64_t sum = (int64_t)((uint64_t)t.sec + (uint64_t)dsec);
  if ((sum > t.sec) == (dsec > 0)) t.sec = sum;
  else if (dsec > 0) t.sec = INT64_MAX;
  else t.sec = -INT64_MAX;
  t.nsec = nsec;
  return t;
}
GoTime go_unix(int64_t sec) { return {(int64_t)((uint64_t)sec + (uint64_t)kUnixToInternal), 0}; }   // time.Unix(sec, 0)
bool go_before(GoTime a, GoTime b) { return a.sec < b.sec || (a.sec == b.sec && a.nsec < b.nsec); }
bool go_after(GoTime a, GoTime b) { return a.sec > b.sec || (a.sec == b.sec && a.nsec > b.nsec); }

double dur_seconds(int64_t d) {                       // time.Duration.Seconds
  const int64_t s = d / kSecond, ns = d % kSecond;
  return (double)s + (double)ns / 1e9;
}
int64_t go_f64_to_i64(double f) {                     // int64(f) on amd64 (CVTTSD2SQ)
  if (std::isnan(f) || f >= 9223372036854775808.0 || f < -9223372036854775808.0) return INT64_MIN;
  return (int64_t)f;
}

// encoding/json field matching: fold(key) == fold(field name) (Go 1.21 foldName)
bool fold_eq(const std::string& key, const char* upper_field) {
  const unsigned char* p = (const unsigned char*)key.data();
  size_t i = 0, j = 0;
  const size_t n = key.size(), m = std::strlen(upper_field);
  while (i < n) {
    if (j >= m) return false;
    uint32_t r;
    size_t w;
    r = json::decode_rune(p + i, n - i, &w);
    if (r >= 'a' && r <= 'z') r -= 32;
    else if (r == 0x17F) r = 'S';          // LATIN SMALL LETTER LONG S folds to S
    else if (r == 0x212A) r = 'K';         // KELVIN SIGN folds to K
    if (r != (unsigned char)upper_field[j]) return false;
    i += w;
    ++j;
  }
  return j == m;
}

}  // namespace

// ====================================================================== Engine
Engine::Engine(const std::vector<int>& devices) : devices_(devices) {
  ctx_ = jg_create(devices.empty() ? nullptr : devices.data(), (int)devices.size());
  if (!ctx_) throw std::runtime_error(std::string("capjwt: no GPU verifier: ") + jg_last_error(nullptr));
  threads_ = host_threads();
}

Engine::~Engine() {
  for (auto& b : pin_free_) jg_host_free(b.first);
  if (ctx_) jg_destroy(ctx_);
}

void Engine::wait_tables() {
  std::shared_lock<std::shared_mutex> life(life_);
  if (ctx_) (void)jg_keys_wait_tables(ctx_);
}

void Engine::load(const std::vector<PublicKey>& keys) {
  std::vector<jg_key> jk;
  jk.reserve(keys.size());
  for (const auto& k : keys) jk.push_back(to_jg(k));
  std::shared_lock<std::shared_mutex> life(life_);
  std::lock_guard<std::mutex> g(load_mu_);
  if (!ctx_) throw DeviceError("capjwt: device lost: " + lost_);
  const int rc = jg_keys_load(ctx_, jk.data(), (int)jk.size());
  if (rc != 0) throw std::runtime_error(std::string("capjwt: jg_keys_load: ") + jg_last_error(ctx_));
  keys_ = keys;
  has_keys_ = true;
}

Engine::Pinned Engine::pinned(size_t bytes) {
  bytes = std::max<size_t>(bytes, 1);
  {
    std::lock_guard<std::mutex> g(pin_mu_);
    // the smallest free block that holds it
    size_t best = pin_free_.size();
    for (size_t i = 0; i < pin_free_.size(); ++i)
      if (pin_free_[i].second >= bytes && (best == pin_free_.size() || pin_free_[i].second < pin_free_[best].second))
        best = i;
    if (best < pin_free_.size()) {
      auto b = pin_free_[best];
      pin_free_.erase(pin_free_.begin() + (std::ptrdiff_t)best);
      return Pinned(this, b.first, b.second);
    }
  }
  // 64 KiB granules, 1/8 headroom: a stream of similar batches reuses one block
  const size_t cap = ((bytes + bytes / 8) + 65535) & ~size_t(65535);
  uint8_t* p = (uint8_t*)jg_host_alloc(cap);
  if (!p) throw std::runtime_error("capjwt: pinned host allocation failed");
  return Pinned(this, p, cap);
}

Engine::Pinned::~Pinned() {
  if (!p_) return;
  std::lock_guard<std::mutex> g(e_->pin_mu_);
  // keep a few blocks (one per concurrent call, typically); drop the smallest beyond that
  e_->pin_free_.emplace_back(p_, cap_);
  if (e_->pin_free_.size() > 4) {
    auto it = std::min_element(e_->pin_free_.begin(), e_->pin_free_.end(),
                               [](const auto& x, const auto& y) { return x.second < y.second; });
    jg_host_free(it->first);
    e_->pin_free_.erase(it);
  }
}

void Engine::fail_device(const std::string& what) {
  errors_.fetch_add(1);
  throw DeviceError(what);
}

void Engine::verify(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, uint8_t* verdicts,
                    const std::function<void()>& submitted) {
  // a lost context: try to recreate it (at most once a second) before failing
  bool lost;
  uint64_t seen;
  {
    std::shared_lock<std::shared_mutex> life(life_);
    lost = ctx_ == nullptr;
    seen = errors_.load();
  }
  if (lost) {
    bool retry;
    {
      std::unique_lock<std::shared_mutex> life(life_);
      retry = std::chrono::steady_clock::now() - last_try_ > std::chrono::seconds(1);
    }
    if (retry) (void)recover(seen + 1);
  }
  std::shared_lock<std::shared_mutex> life(life_);
  if (!ctx_) {
    if (submitted) submitted();
    fail_device("capjwt: device lost: " + lost_);
  }
  jg_ticket* t = nullptr;
  const int rc = jg_submit(ctx_, arena, arena_len, (const jg_tok*)jobs, njobs, verdicts, &t);
  if (submitted) {
    // the device worker reads `jobs` and the arena and writes `verdicts` until
    // jg_wait returns: an exception from the overlapped host work must not
    // unwind the caller's buffers (or return a pooled arena) before that
    try {
      submitted();
    } catch (...) {
      if (rc == 0) (void)jg_wait(ctx_, t);
      throw;
    }
  }
  if (rc == -1) throw std::logic_error(std::string("capjwt: jg_submit rejected the host's jobs: ") + jg_last_error(ctx_));
  if (rc != 0) fail_device(std::string("capjwt: jg_verify_batch: ") + jg_last_error(ctx_));
  const int wc = jg_wait(ctx_, t);
  if (wc == -1) throw std::logic_error(std::string("capjwt: jg_wait rejected the host's jobs: ") + jg_last_error(ctx_));
  if (wc != 0) fail_device(std::string("capjwt: jg_verify_batch: ") + jg_last_error(ctx_));
}

bool Engine::recover(uint64_t seen) {
  std::unique_lock<std::shared_mutex> life(life_);
  if (recovered_at_ >= seen && ctx_) return true;          // already recovered since that error
  last_try_ = std::chrono::steady_clock::now();
  if (ctx_) jg_destroy(ctx_);                              // its streams, workers, staged tables
  ctx_ = jg_create(devices_.empty() ? nullptr : devices_.data(), (int)devices_.size());
  recovered_at_ = errors_.load();
  if (!ctx_) {
    lost_ = std::string("jg_create: ") + jg_last_error(nullptr);
    return false;
  }
  if (has_keys_) {
    std::vector<jg_key> jk;
    jk.reserve(keys_.size());
    for (const auto& k : keys_) jk.push_back(to_jg(k));
    if (jg_keys_load(ctx_, jk.data(), (int)jk.size()) != 0) {
      lost_ = std::string("jg_keys_load: ") + jg_last_error(ctx_);
      jg_destroy(ctx_);
      ctx_ = nullptr;
      return false;
    }
  }
  {
    // the resident sets of the old context, under their ids
    std::lock_guard<std::mutex> g(set_mu_);
    for (int id = 0; id < 16; ++id) {
      if (!sets_[id].live || !sets_[id].stored) continue;
      if (set_load_locked(id) == 0) continue;
      lost_ = std::string("jg_set_load: ") + jg_last_error(ctx_);
      jg_destroy(ctx_);
      ctx_ = nullptr;
      return false;
    }
  }
  lost_.clear();
  recoveries_.fetch_add(1);
  return true;
}

std::string Engine::status() {
  std::shared_lock<std::shared_mutex> life(life_);
  return ctx_ ? std::string() : lost_.empty() ? std::string("device lost") : lost_;
}

int Engine::debug_fail_verify(int n) {
  std::shared_lock<std::shared_mutex> life(life_);
  return ctx_ ? jg_debug_fail_verify(ctx_, n) : -1;
}

// ====================================================================== request coalescing
// Concurrent single-token calls (VerifySignature / Validate) become device
// batches.  A caller pushes its request onto a lock-free stack.  If fewer than
// max_inflight batches are being carried, the caller itself takes everything
// pushed so far (one exchange) and carries it as one batch (parse + device
// verification) -- an idle key set verifies a lone token with no thread
// hand-off; otherwise it sleeps on its own state word.  Dispatcher threads
// (max_inflight of them) serve what the callers leave: whoever finishes a
// batch and finds the stack non-empty wakes one, so pending requests never
// wait for a caller.  Batches pipeline on the device up to max_inflight deep
// and grow with the load.
//
// No lock is taken per call.  A first version (a queue under one mutex, the
// callers leading batches in turn) lost 20x at 1024 callers on a box with 256
// CPUs and a 16-CPU cgroup quota: 243 us of system time per call, the quota
// throttled for most of every period (profiles/r05_s2/session_c.log); the same
// code pinned to 16 CPUs ran 1.2 M calls/s.
namespace {
// process-private futex on a 32-bit word
void futex_wait(void* w, uint32_t expect) {
  syscall(SYS_futex, reinterpret_cast<uint32_t*>(w), FUTEX_WAIT_PRIVATE, expect, nullptr, nullptr, 0);
}
void futex_wake(void* w, int n) {
  syscall(SYS_futex, reinterpret_cast<uint32_t*>(w), FUTEX_WAKE_PRIVATE, n, nullptr, nullptr, 0);
}
}  // namespace

Coalescer::~Coalescer() {
  std::lock_guard<std::mutex> g(threads_mu_);
  stop_locked();
}

void Coalescer::start_locked() {
  stop_.store(false);
  for (int i = 0; i < cfg_.max_inflight; ++i) threads_.emplace_back([this] { dispatch_loop(); });
  started_.store(true, std::memory_order_release);
}

void Coalescer::stop_locked() {
  if (threads_.empty()) return;
  stop_.store(true);
  seq_.fetch_add(1);
  futex_wake(&seq_, INT_MAX);
  for (auto& t : threads_) t.join();
  threads_.clear();
  started_.store(false);
}

void Coalescer::configure(const CoalesceConfig& c) {
  std::lock_guard<std::mutex> g(threads_mu_);
  cfg_ = c;
  cfg_.max_inflight = std::max(1, cfg_.max_inflight);
  cfg_.max_batch = std::max<size_t>(1, cfg_.max_batch);
  cfg_.window_us = std::max<int64_t>(0, cfg_.window_us);
  max_batch_.store(cfg_.max_batch);
  window_us_.store(cfg_.window_us);
  max_inflight_.store(cfg_.max_inflight);
  if (!threads_.empty()) {        // restart with the new count (requests pushed meanwhile wait on the stack)
    stop_locked();
    start_locked();
    kick();
    futex_wake(&seq_, INT_MAX);
  }
}

void Coalescer::kick() {
  seq_.fetch_add(1, std::memory_order_seq_cst);
  futex_wake(&seq_, 1);
}

CoalesceConfig Coalescer::config() {
  std::lock_guard<std::mutex> g(threads_mu_);
  return cfg_;
}

Coalescer::Stats Coalescer::stats() {
  Stats s;
  s.calls = calls_.load();
  s.batches = batches_.load();
  s.max_batch_seen = max_seen_.load();
  return s;
}

// Wake position i of a finished batch's wake-up list
void Coalescer::release(const std::vector<Req*>& wake, size_t i) {
  if (i >= wake.size()) return;
  Req* x = wake[i];
  x->state.store(Req::DONE, std::memory_order_release);
  futex_wake(&x->state, 1);                      // x may be touched no more after this (its owner returns)
}

void Coalescer::run(Req* r) {
  if (!started_.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> g(threads_mu_);
    if (threads_.empty()) start_locked();
  }
  calls_.fetch_add(1, std::memory_order_relaxed);
  Req* h = head_.load(std::memory_order_relaxed);
  do {
    r->next = h;
  } while (!head_.compare_exchange_weak(h, r, std::memory_order_seq_cst, std::memory_order_relaxed));
  if (active_.fetch_add(1, std::memory_order_seq_cst) < max_inflight_.load(std::memory_order_relaxed)) {
    // a free slot: carry everything pushed so far (normally this request too)
    thread_local std::vector<Req*> all, batch;
    serve_stack(all, batch);
    active_.fetch_sub(1, std::memory_order_seq_cst);
    if (head_.load(std::memory_order_seq_cst)) kick();   // what arrived meanwhile: a dispatcher takes it
  } else {
    // every slot busy: whoever finishes a batch finds this request on the stack
    // (the push precedes this caller's view of the slots, which precedes the
    // holder's release, which precedes the holder's look at the stack -- all
    // sequentially consistent).  But the dispatcher that holder kicks may
    // itself be refused by this caller's brief increment and go back to
    // sleep; so if this decrement leaves a slot free while requests wait, kick
    // again.  With every slot truly busy (the heavy-load case) no kick: one
    // futex call per request from 1024 callers cost 25 s of system time per
    // 131 k calls on the box.
    const int prev = active_.fetch_sub(1, std::memory_order_seq_cst);
    if (prev - 1 < max_inflight_.load(std::memory_order_relaxed) && head_.load(std::memory_order_seq_cst)) kick();
  }
  int st;
  while ((st = r->state.load(std::memory_order_acquire)) != Req::DONE) futex_wait(&r->state, (uint32_t)st);
  // carried by a batch: wake this caller's two children in its wake-up tree
  auto peers = std::move(r->peers);
  release(*peers, 2 * r->wpos + 1);
  release(*peers, 2 * r->wpos + 2);
  if (r->ex) std::rethrow_exception(r->ex);
}

void Coalescer::serve_stack(std::vector<Req*>& all, std::vector<Req*>& batch) {
  const int64_t win = window_us_.load(std::memory_order_relaxed);
  if (win > 0) std::this_thread::sleep_for(std::chrono::microseconds(win));
  Req* list = head_.exchange(nullptr, std::memory_order_acquire);
  all.clear();
  for (Req* p = list; p; p = p->next) all.push_back(p);
  std::reverse(all.begin(), all.end());          // oldest first
  const size_t mb = max_batch_.load(std::memory_order_relaxed);
  for (size_t lo = 0; lo < all.size(); lo += mb) {
    batch.assign(all.begin() + (std::ptrdiff_t)lo, all.begin() + (std::ptrdiff_t)std::min(all.size(), lo + mb));
    carry(batch);
  }
}

void Coalescer::dispatch_loop() {
  pthread_setname_np(pthread_self(), "capjwt-batch");
  std::vector<Req*> all, batch;
  while (!stop_.load()) {
    // seq_ is read before the stack and the slots: a kick after this read
    // makes the futex_wait below return at once
    const uint32_t s = seq_.load(std::memory_order_seq_cst);
    if (!head_.load(std::memory_order_seq_cst)) {
      futex_wait(&seq_, s);
      continue;
    }
    if (active_.fetch_add(1, std::memory_order_seq_cst) >= max_inflight_.load(std::memory_order_relaxed)) {
      // every slot busy: the holder kicks when done.  A slot seen busy only
      // through another thread's brief increment is free by now: look again
      // instead of sleeping through the kick that thread may already have sent
      const int prev = active_.fetch_sub(1, std::memory_order_seq_cst);
      if (prev - 1 < max_inflight_.load(std::memory_order_relaxed)) {
        std::this_thread::yield();
        continue;
      }
      futex_wait(&seq_, s);
      continue;
    }
    serve_stack(all, batch);
    active_.fetch_sub(1, std::memory_order_seq_cst);
  }
}

// Run one batch and wake its callers
void Coalescer::carry(std::vector<Req*>& batch) {
  batches_.fetch_add(1, std::memory_order_relaxed);
  uint64_t m = max_seen_.load(std::memory_order_relaxed);
  while (batch.size() > m && !max_seen_.compare_exchange_weak(m, batch.size())) {
  }
  std::exception_ptr ex;
  std::shared_ptr<const Verified> V;
  try {
    std::vector<std::string_view> toks;
    toks.reserve(batch.size());
    for (Req* x : batch) toks.push_back(x->tok);
    V = exec_(toks);
  } catch (...) {
    ex = std::current_exception();
  }
  // the callers wake as a binary tree: the dispatcher wakes the first, each
  // woken caller its own two -- log2(batch) rounds of wake-ups
  auto wake = std::make_shared<std::vector<Req*>>(batch);
  for (size_t i = 0; i < batch.size(); ++i) {
    Req* x = batch[i];
    x->batch = V;
    x->idx = i;
    x->ex = ex;                                  // a host-side bug in the batch reaches every caller in it
    x->wpos = i;
    x->peers = wake;
  }
  release(*wake, 0);
}

// ====================================================================== KeySet
KeySet::KeySet()
    : co_([this](const std::vector<std::string_view>& toks) -> std::shared_ptr<const Verified> {
        return verify_raw(toks);
      }) {}

Results KeySet::verify_batch(const std::vector<std::string_view>& tokens, const PostFn* post) {
  const int th = host_threads();
  Results res(tokens.size(), th);
  // Claims maps are read -- and, with a post step (Validator's claim checks),
  // checked -- while the device verifies (Overlap): a parsed token's payload
  // is JSON-decoded before its verdict is known, and the result of a token no
  // key verifies is replaced afterwards.  pre[i]: 0 not read (finish reads
  // it), 1 read, 2 JSON error (the message in res[i].err), 3 read and post-
  // processed as if verified (kept iff it was).
  std::vector<uint8_t> pre(tokens.size(), 0);
  const Overlap overlap = [&](const Verified& V) {
    parallel_for(tokens.size(), th, [&](size_t lo, size_t hi) {
      auto arena = std::make_unique<json::Arena>();   // this range's claims trees (owned by res)
      json::ArenaScope scope(arena.get());
      res.adopt(std::move(arena));
      std::string jerr;
      for (size_t i = lo; i < hi; ++i) {
        const Tok& t = V.toks[i];
        if (!t.parsed) continue;
        if (claims_map(t.payload, &res[i].claims, &jerr)) {
          pre[i] = 1;
          if (post) {
            res[i].ok = true;
            (*post)(i, res[i], t.view());
            pre[i] = 3;
          }
        } else {
          res[i].claims = json::Value();
          res[i].err = jerr;
          pre[i] = 2;
        }
      }
    });
  };
  std::shared_ptr<Verified> V = verify_raw(tokens, &overlap);
  PhaseTimer pt(trace_name());
  parallel_for(tokens.size(), th, [&](size_t lo, size_t hi) {
    auto arena = std::make_unique<json::Arena>();   // this range's claims trees (owned by res)
    json::ArenaScope scope(arena.get());
    res.adopt(std::move(arena));
    for (size_t i = lo; i < hi; ++i) {
      if (pre[i] == 3) {
        if (!V->failed[i] && V->any[i]) continue;            // verified: the checked result stands
        res[i] = Result();
        finish_pre(*V, i, res[i], true);
      } else if (pre[i]) {
        finish_pre(*V, i, res[i], pre[i] == 1);
      } else {
        finish(*V, i, res[i]);
      }
      if (post) (*post)(i, res[i], V->toks[i].view());
    }
  });
  pt.lap("payload-json");
  V->toks.release();
  pt.lap("free-toks");
  return res;
}

// One token of a coalesced batch: the leader ran parse + device verify for
// everyone; the claims map is built here, on the caller's own thread, straight
// into heap storage (it leaves the batch with the caller)
Result KeySet::VerifySignature(std::string_view token) {
  Coalescer::Req q;
  q.tok = token;
  co_.run(&q);
  Result r;
  finish(*q.batch, q.idx, r);
  return r;
}

Result KeySet::verify_one(std::string_view token, TokenInfo* info) {
  Coalescer::Req q;
  q.tok = token;
  co_.run(&q);
  Result r;
  finish(*q.batch, q.idx, r);
  const TokenView t = q.batch->toks[q.idx].view();
  info->parsed = t.parsed;
  info->parse_err = std::string(t.parse_err);
  info->nsigs = t.nsigs;
  info->sig0_len = t.sig0_len;
  info->alg = std::string(t.alg);
  return r;
}

Results KeySet::VerifySignatureBatch(const std::vector<std::string_view>& tokens) {
  return verify_batch(tokens, nullptr);
}

std::unique_ptr<KeySet> NewStaticKeySet(const std::vector<PublicKey>& keys, std::string* err,
                                        const std::vector<int>& devices) {
  if (keys.empty()) { *err = "publicKeys must not be empty"; return nullptr; }
  if (keys.size() > 65535) { *err = "at most 65535 keys"; return nullptr; }
  return std::make_unique<StaticKeySet>(keys, devices);
}

std::unique_ptr<KeySet> NewJSONWebKeySet(const std::string& jwks_url, const std::string& jwks_ca_pem, Fetcher fetch,
                                         std::string* err, const std::vector<int>& devices) {
  if (jwks_url.empty()) { *err = "jwksURL must not be empty"; return nullptr; }
  if (!jwks_ca_pem.empty() && !ca_pem_ok(jwks_ca_pem)) { *err = "could not parse CA PEM value successfully"; return nullptr; }
  return std::make_unique<JSONWebKeySet>(jwks_url, jwks_ca_pem, std::move(fetch), devices);
}

// go-oidc's oidc.KeySet over the same GPU JWKS machinery
class RemoteKeySet::Impl {
 public:
  Impl(const std::string& url, Fetcher f, const std::vector<int>& devices)
      : ks(url, "", std::move(f), devices),
        co([this](const std::vector<std::string_view>& toks) -> std::shared_ptr<const Verified> {
          return ks.verify_raw(toks);
        }) {}
  JSONWebKeySet ks;
  Coalescer co;
};
RemoteKeySet::RemoteKeySet(const std::string& jwks_url, Fetcher fetch, const std::vector<int>& devices)
    : impl_(std::make_unique<Impl>(jwks_url, std::move(fetch), devices)) {}
RemoteKeySet::~RemoteKeySet() = default;
PayloadResult RemoteKeySet::VerifySignature(std::string_view jwt) {
  Coalescer::Req q;
  q.tok = jwt;
  impl_->co.run(&q);
  return JSONWebKeySet::payload_result(*q.batch, q.idx);
}
std::vector<PayloadResult> RemoteKeySet::VerifySignatureBatch(const std::vector<std::string_view>& jwts) {
  return impl_->ks.verify_payload_batch(jwts);
}
void RemoteKeySet::SetCoalescing(const CoalesceConfig& c) { impl_->co.configure(c); }
std::unique_ptr<RemoteKeySet> NewRemoteKeySet(const std::string& jwks_url, Fetcher fetch,
                                              const std::vector<int>& devices) {
  return std::make_unique<RemoteKeySet>(jwks_url, std::move(fetch), devices);
}

std::unique_ptr<KeySet> NewOIDCDiscoveryKeySet(const std::string& issuer, const std::string& issuer_ca_pem,
                                               Fetcher fetch, std::string* err, const std::vector<int>& devices) {
  // jwt/keyset.go:49-104
  if (issuer.empty()) { *err = "issuer must not be empty"; return nullptr; }
  if (!issuer_ca_pem.empty() && !ca_pem_ok(issuer_ca_pem)) { *err = "could not parse CA PEM value successfully"; return nullptr; }
  std::string base = issuer;
  if (!base.empty() && base.back() == '/') base.pop_back();          // strings.TrimSuffix(issuer, "/")
  FetchResponse resp;
  try {
    resp = fetch(base + "/.well-known/openid-configuration", issuer_ca_pem);
  } catch (const std::exception& e) {
    *err = e.what();
    return nullptr;
  }
  if (resp.status != 200) { *err = resp.status_text + ": " + resp.body; return nullptr; }
  json::Value doc;
  std::string jerr;
  std::string iss, jwks;
  bool ok = json::parse(resp.body, &doc, &jerr);
  if (ok && !doc.is_null() && doc.kind != json::Value::Object) { ok = false; jerr = "json: cannot unmarshal into struct"; }
  if (ok && doc.kind == json::Value::Object) {
    // encoding/json into struct { Issuer `json:"issuer"`; JWKSURL `json:"jwks_uri"` }
    for (const auto& m : doc.obj) {
      std::string* dst = fold_eq(m.first, "ISSUER") ? &iss : fold_eq(m.first, "JWKS_URI") ? &jwks : nullptr;
      if (!dst || m.second.is_null()) continue;
      if (m.second.kind != json::Value::String) { ok = false; jerr = "json: cannot unmarshal into string"; break; }
      *dst = m.second.str;
    }
  }
  if (!ok) {
    // unmarshalResp (jwt/keyset.go:229-241)
    std::string media = resp.content_type.substr(0, resp.content_type.find(';'));
    while (!media.empty() && media.back() == ' ') media.pop_back();
    for (auto& c : media) c = (char)std::tolower((unsigned char)c);
    if (media == "application/json")
      *err = "failed to decode OIDC discovery document: got Content-Type = application/json, but could not unmarshal as JSON: " + jerr;
    else
      *err = "failed to decode OIDC discovery document: expected Content-Type = application/json, got \"" +
             resp.content_type + "\": " + jerr;
    return nullptr;
  }
  if (iss != issuer) {
    *err = "issuer did not match the returned issuer, expected \"" + issuer + "\" got \"" + iss + "\"";
    return nullptr;
  }
  return std::make_unique<JSONWebKeySet>(jwks, issuer_ca_pem, std::move(fetch), devices);
}

bool ParsePublicKeyPEM(std::string_view data, PublicKey* out, std::string* err) {
  return parse_public_key_pem(data, out, err);
}

// ====================================================================== Validator
std::unique_ptr<Validator> NewValidator(KeySet* ks, std::string* err) {
  if (!ks) { *err = "keySet must not be nil"; return nullptr; }
  return std::make_unique<Validator>(ks);
}

namespace {
// The jwt.Claims field a claims-map member lands in under encoding/json's
// case-insensitive matching (fold_eq).  Every field name is 3 letters: a
// 3-byte ASCII key is matched by upper-casing it; a key with non-ASCII runes
// (the 'ſ' and Kelvin-sign foldings) takes fold_eq.
enum ClaimField { F_NONE, F_ISS, F_SUB, F_JTI, F_AUD, F_EXP, F_NBF, F_IAT };
ClaimField claim_field(const std::string& key) {
  static const char* const names[] = {"", "ISS", "SUB", "JTI", "AUD", "EXP", "NBF", "IAT"};
  const size_t n = key.size();
  if (n < 3 || n > 9) return F_NONE;         // 3 runes of 1..3 bytes
  if (n == 3) {
    char u[3];
    for (int i = 0; i < 3; ++i) {
      const unsigned char c = (unsigned char)key[i];
      if (c >= 0x80) return F_NONE;          // a multi-byte rune cannot fit 3 bytes with 2 more
      u[i] = (char)(c >= 'a' && c <= 'z' ? c - 32 : c);
    }
    for (int f = F_ISS; f <= F_IAT; ++f)
      if (u[0] == names[f][0] && u[1] == names[f][1] && u[2] == names[f][2]) return (ClaimField)f;
    return F_NONE;
  }
  for (int f = F_ISS; f <= F_IAT; ++f)
    if (fold_eq(key, names[f])) return (ClaimField)f;
  return F_NONE;
}
}  // namespace

Leeways resolve_leeways(const Expected& expected) {
  Leeways l;
  auto seconds = [](int64_t d) {
    double lw = dur_seconds(d);
    if (lw < 0) lw = 0;
    else if (lw == 0) lw = DefaultLeewaySeconds;
    return go_f64_to_i64(lw);
  };
  l.exp_s = seconds(expected.ExpirationLeeway);
  l.nbf_s = seconds(expected.NotBeforeLeeway);
  l.skew_ns = expected.ClockSkewLeeway;
  if (dur_seconds(l.skew_ns) < 0) l.skew_ns = 0;
  else if (dur_seconds(l.skew_ns) == 0) l.skew_ns = 60 * kSecond;   // jwt.DefaultLeeway = 1 minute
  return l;
}

namespace {
// validateSigningAlgorithm (jwt/jwt.go:207-239)  [R36]: "" or Validate's error
std::string alg_header_error(const TokenView& info, const Expected& expected) {
  std::string e = SupportedSigningAlgorithm(expected.SigningAlgorithms);
  if (e.empty() && !info.parsed) e = std::string(info.parse_err);
  if (e.empty() && (info.nsigs == 0 || (info.nsigs == 1 && info.sig0_len == 0))) e = "token must be signed";
  if (e.empty() && info.nsigs > 1) e = "token with multiple signatures not supported";
  if (e.empty()) {
    bool found = false;
    if (expected.SigningAlgorithms.empty()) found = info.alg == "RS256";
    for (const auto& a : expected.SigningAlgorithms) found = found || a == info.alg;
    if (!found) e = "token signed with unexpected algorithm";
  }
  return e.empty() ? e : "invalid algorithm (alg) header parameter: " + e;
}
}  // namespace

Result validate_claims(const json::Value& all_claims, const TokenInfo& info, const Expected& expected,
                       int64_t now_unix_ns) {
  return validate_claims(all_claims, TokenView{info.parsed, info.parse_err, info.nsigs, info.sig0_len, info.alg},
                         expected, now_unix_ns);
}

Result validate_claims(const json::Value& all_claims, const TokenView& info, const Expected& expected,
                       int64_t now_unix_ns) {
  return validate_claims(all_claims, info, expected, now_unix_ns, nullptr);
}

Result validate_claims(const json::Value& all_claims, const TokenView& info, const Expected& expected,
                       int64_t now_unix_ns, RegisteredClaims* decoded) {
  Result r;
  r.err = alg_header_error(info, expected);
  if (!r.err.empty()) return r;
  // json.Marshal(allClaims) -> json.Unmarshal(&jwt.Claims{})  [R37]: members in
  // sorted key order, each assigned to the case-insensitively matching field.
  // The fields are views into all_claims (which outlives this call).
  std::string_view iss, sub, jti;
  const json::Value* aud = nullptr;            // a String, or an Array of Strings
  bool has_iat = false, has_exp = false, has_nbf = false;
  int64_t iat = 0, exp = 0, nbf = 0;
  if (all_claims.kind == json::Value::Object) {
    const json::Member* small[32];
    std::vector<const json::Member*> big;
    const json::Member** ms = small;
    const size_t nm = all_claims.obj.size();
    if (nm > 32) {
      big.resize(nm);
      ms = big.data();
    }
    for (size_t k = 0; k < nm; ++k) ms[k] = &all_claims.obj[k];
    std::sort(ms, ms + nm, [](const json::Member* a, const json::Member* b) { return a->first < b->first; });
    for (size_t mk = 0; mk < nm; ++mk) {
      const json::Member* m = ms[mk];
      const json::Value& v = m->second;
      const ClaimField f = claim_field(m->first);
      if (f == F_NONE) continue;
      if (f == F_ISS || f == F_SUB || f == F_JTI) {
        if (v.is_null()) continue;
        if (v.kind != json::Value::String) {
          r.err = "json: cannot unmarshal into Go struct field Claims." + m->first + " of type string";
          return r;
        }
        (f == F_ISS ? iss : f == F_SUB ? sub : jti) = v.str;
        continue;
      }
      if (f == F_AUD) {
        // jwt.Audience.UnmarshalJSON: string or array of strings; null included
        bool ok = v.kind == json::Value::String || v.kind == json::Value::Array;
        if (v.kind == json::Value::Array)
          for (const auto& e : v.arr)
            if (e.kind != json::Value::String) { ok = false; break; }
        if (!ok) {
          r.err = "square/go-jose/jwt: expected string or array value to unmarshal to Audience";
          return r;
        }
        aud = &v;
        continue;
      }
      bool* has = f == F_EXP ? &has_exp : f == F_NBF ? &has_nbf : &has_iat;
      int64_t* dst = f == F_EXP ? &exp : f == F_NBF ? &nbf : &iat;
      if (v.is_null()) { *has = false; *dst = 0; continue; }       // *NumericDate = nil
      if (v.kind != json::Value::Number) {
        r.err = "square/go-jose/jwt: expected number value to unmarshal NumericDate";
        return r;
      }
      *has = true;
      *dst = go_f64_to_i64(v.num);                                 // NumericDate(f)
    }
  }
  if (decoded) {
    decoded->Issuer = std::string(iss);
    decoded->Subject = std::string(sub);
    decoded->ID = std::string(jti);
    decoded->Audience.clear();
    if (aud && aud->kind == json::Value::String) decoded->Audience.emplace_back(aud->str.view());
    else if (aud)
      for (const auto& a : aud->arr) decoded->Audience.emplace_back(a.str.view());
    decoded->Expiry = has_exp ? std::optional<int64_t>(exp) : std::nullopt;
    decoded->NotBefore = has_nbf ? std::optional<int64_t>(nbf) : std::nullopt;
    decoded->IssuedAt = has_iat ? std::optional<int64_t>(iat) : std::nullopt;
  }
  // time defaulting (jwt/jwt.go:117-170)  [R38]
  if (!has_iat) iat = 0;
  if (!has_exp) exp = 0;
  if (!has_nbf) nbf = 0;
  if (iat == 0 && exp == 0 && nbf == 0) {
    r.err = "no issued at (iat), not before (nbf), or expiration time (exp) claims in token";
    return r;
  }
  const Leeways lw = resolve_leeways(expected);
  if (exp == 0) {
    const int64_t latest = nbf > iat ? nbf : iat;
    exp = (int64_t)((uint64_t)latest + (uint64_t)lw.exp_s);
  }
  if (nbf == 0) {
    if (iat != 0) nbf = iat;
    else nbf = (int64_t)((uint64_t)exp - (uint64_t)lw.nbf_s);
  }
  const int64_t cks = lw.skew_ns;
  // registered claims (jwt/jwt.go:172-184)  [R39]
  if (!expected.Issuer.empty() && expected.Issuer != iss) { r.err = "invalid issuer (iss) claim"; return r; }
  if (!expected.Subject.empty() && expected.Subject != sub) { r.err = "invalid subject (sub) claim"; return r; }
  if (!expected.ID.empty() && expected.ID != jti) { r.err = "invalid ID (jti) claim"; return r; }
  if (!expected.Audiences.empty()) {
    bool found = false;
    for (const auto& e : expected.Audiences) {
      if (!aud) break;
      if (aud->kind == json::Value::String) found = found || aud->str == e;
      else
        for (const auto& a : aud->arr) found = found || a.str == e;
    }
    if (!found) {
      r.err = "invalid audience (aud) claim: audience claim does not match any expected audience";
      return r;
    }
  }
  // time window (jwt/jwt.go:186-199)
  const GoTime now = go_now(now_unix_ns);
  if (go_before(go_add(now, cks), go_unix(nbf))) { r.err = "invalid not before (nbf) claim: token not yet valid"; return r; }
  if (go_after(go_add(now, -cks), go_unix(exp))) { r.err = "invalid expiration time (exp) claim: token is expired"; return r; }
  if (go_before(go_add(now, cks), go_unix(iat))) { r.err = "invalid issued at (iat) claim: token issued in the future"; return r; }
  r.ok = true;                 // the caller attaches all_claims (returned unchanged)
  return r;
}

void release_results(Results& rs) { rs.release(); }

// jwt/jwt.go:95-202 for one token: the signature through the key set's
// coalescer (concurrent Validate calls share device batches), the claim
// checks on the caller's thread with the caller's Expected
Result Validator::Validate(std::string_view token, const Expected& expected) {
  TokenInfo info;
  Result r = ks_->verify_one(token, &info);
  if (!r.ok) {
    r.err = "error verifying token signature: " + r.err;
    return r;
  }
  const int64_t now = expected.has_now ? expected.now_unix_ns : wall_now_ns();
  Result v = validate_claims(r.claims, info, expected, now);
  if (v.ok) v.claims = std::move(r.claims);
  return v;
}

Results Validator::ValidateBatch(const std::vector<std::string_view>& tokens, const Expected& expected) {
  const int64_t now = expected.has_now ? expected.now_unix_ns : wall_now_ns();
  // the claim checks run inside the key set's per-token pass, on the host
  // threads, while each token's claims map is still in cache; a claims map
  // that fails validation is destroyed there
  const PostFn post = [&](size_t, Result& r, const TokenView& t) {
    if (!r.ok) {
      r.err = "error verifying token signature: " + r.err;
      return;
    }
    Result v = validate_claims(r.claims, t, expected, now);
    if (v.ok) v.claims = std::move(r.claims);
    r = std::move(v);
  };
  return ks_->verify_batch(tokens, &post);
}

namespace {
// the string Validate gives for a jg_claim_code (jwt/jwt.go:117-199)
const char* claim_code_error(uint8_t code) {
  switch (code) {
    case JG_CL_NO_TIME: return "no issued at (iat), not before (nbf), or expiration time (exp) claims in token";
    case JG_CL_ISS: return "invalid issuer (iss) claim";
    case JG_CL_SUB: return "invalid subject (sub) claim";
    case JG_CL_JTI: return "invalid ID (jti) claim";
    case JG_CL_AUD: return "invalid audience (aud) claim: audience claim does not match any expected audience";
    case JG_CL_NBF: return "invalid not before (nbf) claim: token not yet valid";
    case JG_CL_EXP: return "invalid expiration time (exp) claim: token is expired";
    case JG_CL_IAT: return "invalid issued at (iat) claim: token issued in the future";
    default: return "";
  }
}
}  // namespace

// ---- ClaimSet: what a handle shares ----
// The host copy: immutable parts, parts[0] the base and the rest what ClaimSet::Add
// has added since, disjoint.  A snapshot (MatchPlan) shares the parts; an Add makes
// a new HostSet of the same parts and one more, never a copy of the members: two
// trailing parts of like size are merged (as a binary counter carries, so there
// are O(log n) parts and an Add of k members costs O(k) amortised), and all are
// folded into a new base once those added pass one eighth of it.
struct HostSet {
  using Part = std::unordered_set<std::string>;
  std::vector<std::shared_ptr<const Part>> parts;
  size_t n = 0;
  size_t size() const { return n; }
  size_t count(const std::string& m) const {
    for (const auto& p : parts)
      if (p->count(m)) return 1;
    return 0;
  }
  static std::shared_ptr<const HostSet> of(Part&& base) {
    auto h = std::make_shared<HostSet>();
    h->n = base.size();
    h->parts.push_back(std::make_shared<const Part>(std::move(base)));
    return h;
  }
  // this set and `fresh`, none of which it holds
  std::shared_ptr<const HostSet> with(Part&& fresh) const {
    auto h = std::make_shared<HostSet>(*this);
    h->n += fresh.size();
    h->parts.push_back(std::make_shared<const Part>(std::move(fresh)));
    const auto merge_last = [&h] {
      Part u(*h->parts[h->parts.size() - 2]);
      u.insert(h->parts.back()->begin(), h->parts.back()->end());
      h->parts.pop_back();
      h->parts.back() = std::make_shared<const Part>(std::move(u));
    };
    while (h->parts.size() > 2 && 2 * h->parts.back()->size() >= h->parts[h->parts.size() - 2]->size()) merge_last();
    if (8 * (h->n - h->parts[0]->size()) > h->parts[0]->size())
      while (h->parts.size() > 1) merge_last();
    return h;
  }
};
struct ClaimSetImpl {
  Engine* eng = nullptr;
  int id = -1;
  uint32_t token = 0;
  std::mutex mu;                                      // host, host_only, closed
  std::shared_ptr<const HostSet> host;
  bool host_only = false, closed = false;
  ~ClaimSetImpl() {
    if (!closed && eng && id >= 0) eng->set_release(id);
  }
};

namespace {
// Appends bytes [off, off + len) of the payload that `seg` (canonical unpadded
// base64url: the scan decided it) encodes, decoding only the characters that
// carry them: [4 (off / 3), 4 ceil((off + len) / 3)).
void append_span(std::string& out, std::string_view seg, uint32_t off, uint32_t len) {
  // kTrip[k][c]: the sextet of character c, shifted to its place in a group's 24 bits
  struct Tables {
    uint32_t t[4][256];
  };
  static const Tables kTrip = [] {
    Tables T{};
    const char* abc = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_";
    for (int k = 0; k < 4; ++k)
      for (uint32_t v = 0; v < 64; ++v) T.t[k][(uint8_t)abc[v]] = v << (18 - 6 * k);
    return T;
  }();
  if (len == 0) return;
  const size_t g0 = off / 3, g1 = ((size_t)off + len + 2) / 3;     // groups of 4 characters -> 3 bytes
  const size_t skip = off - 3 * g0, base = out.size();
  out.resize(base + 3 * (g1 - g0));
  char* w = &out[base];
  const uint8_t* p = (const uint8_t*)seg.data();
  const size_t whole = std::min(g1, seg.size() / 4);               // groups with all four characters
  size_t g = g0;
  for (; g < whole; ++g, w += 3) {
    const uint32_t trip = kTrip.t[0][p[4 * g]] | kTrip.t[1][p[4 * g + 1]] | kTrip.t[2][p[4 * g + 2]] | kTrip.t[3][p[4 * g + 3]];
    w[0] = (char)(trip >> 16);
    w[1] = (char)(trip >> 8);
    w[2] = (char)trip;
  }
  for (; g < g1; ++g, w += 3) {                                    // the segment's last, short group
    uint32_t trip = 0;
    for (size_t k = 0; k < 4 && 4 * g + k < seg.size(); ++k) trip |= kTrip.t[k][p[4 * g + k]];
    w[0] = (char)(trip >> 16);
    w[1] = (char)(trip >> 8);
    w[2] = (char)trip;
  }
  if (skip) std::memmove(&out[base], &out[base + skip], len);
  out.resize(base + len);
}

// The elements of an aud value's text, "s" or [ "a", "b" ]: no escapes (the
// scan decided it), so they are the quoted runs.  each(begin, length)
template <class F>
void aud_elements(std::string_view text, F&& each) {
  for (size_t q = text.find('"'); q != std::string_view::npos; q = text.find('"', q + 1)) {
    const size_t e = text.find('"', q + 1);
    if (e == std::string_view::npos) break;
    each(q + 1, e - q - 1);
    q = e;
  }
}

// jwt.Claims from the scan's record of a payload it decided
RegisteredClaims claims_of_record(std::string_view seg, const jg_claims& v) {
  RegisteredClaims c;
  append_span(c.Issuer, seg, v.iss_off, v.iss_len);
  append_span(c.Subject, seg, v.sub_off, v.sub_len);
  append_span(c.ID, seg, v.jti_off, v.jti_len);
  if (v.aud_n) {
    std::string text;
    append_span(text, seg, v.aud_off, v.aud_len);
    c.Audience.reserve(v.aud_n);
    aud_elements(text, [&](size_t at, size_t n) { c.Audience.emplace_back(text, at, n); });
  }
  if ((v.present >> 5) & 1u) c.Expiry = v.exp;
  if ((v.present >> 6) & 1u) c.NotBefore = v.nbf;
  if ((v.present >> 7) & 1u) c.IssuedAt = v.iat;
  return c;
}

// CheckBatch's flow.  X = false: put(i, ok, err) receives token i's outcome
// once, from a host thread (CheckBatch keeps the strings, CheckVerdicts only
// the bit).  X = true (RegisteredBatch): the scan is jg_claims_extract, its
// records lie behind the jobs in the same pinned block, and `put` is a sink
// that receives each token once: reject(chunk, i, err); record(chunk, i,
// payload segment, jg_claims) for a token the device accepted;
// claims(chunk, i, jwt.Claims) for one the host path accepted.  chunk: which of
// make_chunks(n, host_threads())'s ranges i lies in; one thread per chunk, in
// index order.  M = kSelectMode (SelectBatch): the scan is jg_claims_select with
// the caller's names (`select`; nullptr: a name list the ABI does not take, every
// token takes the host path), the jg_selected records lie behind the jg_claims
// records, record(...) also receives token i's jg_selected and claims(...) the
// verified claims map of the host-path token.  M = kPathMode: kSelectMode with
// the caller's paths (`paths`, nullptr as for `select`) and jg_claims_paths as
// the scan, with one Expected too (a table of one profile).  M = kMatchMode
// (MatchBatch): kCheckMode with jg_claims_match as the scan (`match`: its paths
// and predicates, or not scannable: every token takes the host path) and a mask
// per token behind the jobs; put(i, ok, err, bits) also receives the mask of an
// accepted token -- the scan's, or match_requires() on the verified claims map.
constexpr int kCheckMode = 0, kRegisteredMode = 1, kSelectMode = 2, kPathMode = 3, kMatchMode = 4;

// The requirements of a MatchBatch call as the scan takes them (jg_paths and
// jg_preds): equal paths share a slot, equal requirements a predicate (bit[k]:
// the scan's bit for requires[k]).  usable == false: the ABI does not take the
// list and every token goes the host path.
struct MatchPlan {
  const std::vector<Require>& reqs;
  std::string names, values;
  jg_paths paths{};
  jg_preds preds{};
  std::vector<int> bit;
  bool usable = true;
  bool identity = true;                              // bit[k] == k for every k: the scan's mask is the caller's
  explicit MatchPlan(const std::vector<Require>& reqs);
  // The MatchBatchArgs entries: the requirements may take operands, n per column.  The operands travel as a
  // jg_args (job-major spans into `abytes`, numbers in `anums`); host_only[i]: token i has a string operand the
  // scan refuses, so it is not scanned and its spans are empty.
  MatchPlan(const std::vector<Require>& reqs, size_t n, const std::vector<std::vector<std::string_view>>& strs,
            const std::vector<const int64_t*>& nums, bool with_args = true,
            const std::vector<HashColumn>* hashes = nullptr);
  bool with_args = false;
  const std::vector<std::vector<std::string_view>>* strs = nullptr;
  const std::vector<const int64_t*>* nums = nullptr;
  std::string abytes;
  std::vector<jg_sarg> aspans;
  std::vector<int64_t> anums;
  std::vector<uint8_t> host_only;
  jg_args args{};
  // The hash columns (jg_claims_match_hash), with_hash: the call has one, or a HashOfArg or IsString.  The
  // values travel as a jg_hargs (job-major spans into `hbytes`); a token whose value is over JG_HASH_SRC_MAX is
  // host_only.  The family of a span is its token's alg's, known once the batch is parsed: set_families().
  bool with_hash = false;
  bool hash_reqs = false;                             // a HashOfArg among the requirements
  const std::vector<HashColumn>* hashes = nullptr;
  std::string hbytes;
  mutable std::vector<jg_hsrc> hsrc;
  jg_hargs hargs{};
  // host path: hosted[i * nhash + c] is what token i's claim must equal under hash column c, "" for none
  mutable std::vector<std::string> hosted;
  // The resident sets (jg_claims_match_set), with_sets: an InSet or AnyElementIn among the requirements.  The
  // distinct handles are the call's set indices, at most JG_MAX_SETS of them and none host-only, or the list is
  // not usable; snaps[k] is the host copy requirement k is held to on the host path, taken when the plan is made.
  bool with_sets = false;
  std::vector<std::shared_ptr<ClaimSetImpl>> set_impls;
  std::vector<std::shared_ptr<const HostSet>> snaps;
  jg_setargs sets{};
  // token i's operands for the host path
  uint32_t host_bits(const json::Value& claims, size_t i) const;
  // the caller's mask from the scan's
  uint32_t spread(uint32_t m) const {
    if (identity) return m;
    uint32_t out = 0;
    for (size_t k = 0; k < bit.size(); ++k) out |= ((m >> bit[k]) & 1u) << k;
    return out;
  }
};

int hash_fam_of_alg(int alg);                        // the SHA-2 of a token's hash claims, below

// One Expected as the scan takes it (include/jg.h jg_expect) and the clock its
// tokens are held to.  scannable == false: one the ABI does not take (more than
// JG_MAX_AUD audiences, strings over JG_EXPECT_MAX_BYTES); its tokens take the
// host path.
struct ScanProfile {
  jg_expect ex{};
  std::string strs;
  int64_t now = 0;
  bool scannable = false;
};
void resolve_scan_profile(const Expected& expected, int64_t now, ScanProfile* P) {
  jg_expect& ex = P->ex;
  P->now = now;
  P->strs = expected.Issuer + expected.Subject + expected.ID;
  ex.iss_len = (uint32_t)expected.Issuer.size();
  ex.sub_len = (uint32_t)expected.Subject.size();
  ex.jti_len = (uint32_t)expected.ID.size();
  bool scannable = expected.Audiences.size() <= JG_MAX_AUD;
  if (scannable) {
    ex.naud = (uint32_t)expected.Audiences.size();
    for (size_t k = 0; k < expected.Audiences.size(); ++k) {
      ex.aud_len[k] = (uint32_t)expected.Audiences[k].size();
      P->strs += expected.Audiences[k];
    }
  }
  P->scannable = scannable && P->strs.size() <= JG_EXPECT_MAX_BYTES;
  ex.strs = (const uint8_t*)P->strs.data();
  int64_t s = now / kSecond, ns = now % kSecond;
  if (ns < 0) { ns += kSecond; --s; }
  ex.now_sec = s;
  ex.now_nsec = (uint32_t)ns;
  const Leeways lw = resolve_leeways(expected);
  ex.skew_ns = lw.skew_ns;
  ex.exp_leeway_s = lw.exp_s;
  ex.nbf_leeway_s = lw.nbf_s;
}

// Each = false: one Expected (exps[0]) for every token, `which` unused -- the
// six entries above.  Each = true (the *Each entries): token i is held to
// exps[which[i]]: its clock, leeways, SigningAlgorithms and expected strings;
// one signature submission and one scan call (jg_claims_each) for the batch.
// Profiles get device slots in index order while they fit (scannable, fewer than
// JG_MAX_PROFILES slots taken, JG_PROFILE_POOL_BYTES of strings in all); the
// tokens of a profile without a slot are not scanned and take the host path,
// as every token of an unscannable Expected does, so no result depends on the caps.
template <int M, bool Each, class Put>
void check_core(KeySet* ks_, const std::vector<std::string_view>& tokens, const Expected* exps, size_t nexp,
                const uint32_t* which, CheckStats* stats, Put&& put, const jg_select* select = nullptr,
                const jg_paths* paths = nullptr, const MatchPlan* match = nullptr) {
  constexpr bool X = M >= kRegisteredMode && M != kMatchMode;
  // a token that is not accepted carries no claims
  auto reject = [&](size_t c, size_t i, std::string&& err) {
    if constexpr (X) put.reject(c, i, std::move(err));
    else if constexpr (M == kMatchMode) put(i, false, std::move(err), 0u);
    else put(i, false, std::move(err));
  };
  const size_t n = tokens.size();
  const int th = host_threads();
  // the profiles of the scan and slot[p], profile p's index in the call's
  // table (exs) or -1; the wall clock is read once
  std::vector<ScanProfile> prof(nexp);
  std::vector<int32_t> slot(nexp, -1);
  std::vector<jg_expect> exs;
  {
    bool have_wall = false;
    int64_t wall = 0;
    size_t pool = 0;
    for (size_t p = 0; p < nexp; ++p) {
      if (!exps[p].has_now && !have_wall) {
        wall = wall_now_ns();
        have_wall = true;
      }
      resolve_scan_profile(exps[p], exps[p].has_now ? exps[p].now_unix_ns : wall, &prof[p]);
      bool fits = prof[p].scannable;
      if constexpr (M == kSelectMode) fits = fits && select != nullptr;
      if constexpr (M == kPathMode) fits = fits && paths != nullptr;
      if constexpr (M == kMatchMode) fits = fits && match->usable;
      if constexpr (Each)
        fits = fits && exs.size() < JG_MAX_PROFILES && pool + prof[p].strs.size() <= JG_PROFILE_POOL_BYTES;
      if (!fits) continue;
      slot[p] = (int32_t)exs.size();
      pool += prof[p].strs.size();
      exs.push_back(prof[p].ex);
    }
  }
  const bool scannable = !exs.empty();
  // code[i]: the device's verdict on token i's registered claims; JG_CL_HOST
  // also for a token that was never scanned.  Job i is token i's payload
  // segment inside the arena the signatures are verified from (a canonical
  // compact token is copied there as it is); len 0 = not in the arena.
  // Both arrays live in one pinned block of the engine's pool (DMA at link
  // speed, no page faults in steady state).
  Engine& eng = ks_->engine();
  if constexpr (M == kMatchMode)
    for (const auto& si : match->set_impls)
      if (si->eng != &eng) throw std::invalid_argument("capjwt: a claim set of another key set");
  const size_t rec_bytes = X ? n * sizeof(jg_claims) : 0;      // jobs | records | selected | masks | codes
  const size_t sel_bytes = X && M >= kSelectMode ? n * sizeof(jg_selected) : 0;
  const size_t mask_bytes = M == kMatchMode ? n * sizeof(uint32_t) : 0;
  Engine::Pinned scanbuf = eng.pinned(n * (sizeof(jg_cjob) + 1) + rec_bytes + sel_bytes + mask_bytes + 16);
  jg_cjob* const jobs = (jg_cjob*)scanbuf.get();
  jg_claims* const recs = (jg_claims*)(scanbuf.get() + n * sizeof(jg_cjob));
  jg_selected* const sels = (jg_selected*)(scanbuf.get() + n * sizeof(jg_cjob) + rec_bytes);
  uint32_t* const masks = (uint32_t*)(scanbuf.get() + n * sizeof(jg_cjob) + rec_bytes + sel_bytes);
  uint8_t* const code = scanbuf.get() + n * sizeof(jg_cjob) + rec_bytes + sel_bytes + mask_bytes;
  (void)masks;
  std::memset(code, JG_CL_HOST, n);
  bool have_jobs = false;
  bool scan_failed = false;
  std::string scan_err;
  uint64_t scan_seen = 0;
  const KeySet::Overlap overlap = [&](const Verified& V) {
    if (!scannable || !V.arena || n == 0) return;
    PhaseTimer pt("check");
    have_jobs = true;
    parallel_for(n, th, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        const Tok& t = V.toks[i];
        jg_cjob& j = jobs[i];
        j.off = 0;
        j.len = 0;
        j.flags = 0;
        if (!t.ncand || !t.lit) continue;
        if constexpr (M == kMatchMode)
          if (match->with_args && match->host_only[i]) continue;   // an operand the scan refuses: the host path
        if constexpr (Each) {
          const int32_t sl = slot[which[i]];
          if (sl < 0) continue;                           // no slot: the host path
          j.flags = (uint32_t)sl;
        }
        const char* dot = (const char*)std::memchr(t.lit, '.', t.si_len);
        if (!dot) continue;
        const size_t d1 = (size_t)(dot - t.lit);
        j.off = V.jobs[t.job0].off + d1 + 1;
        j.len = (uint32_t)(t.si_len - d1 - 1);
      }
    });
    pt.lap("scan-jobs");
    try {
      const jg_expect& ex = exs[0];
      if constexpr (M == kMatchMode) {
        if (match->with_hash || match->with_sets) {
          // a value is hashed with the SHA-2 of its token's alg; a token that is not scanned has no value here
          const size_t nh = match->hargs.nhash;
          if (nh)
            parallel_for(n, th, [&](size_t lo, size_t hi) {
              for (size_t i = lo; i < hi; ++i)
                for (size_t c = 0; c < nh; ++c) {
                  jg_hsrc& s = match->hsrc[i * nh + c];
                  if (s.fam) s.fam = (uint8_t)(jobs[i].len ? hash_fam_of_alg(V.toks[i].alg) : 0);
                }
            });
          if (match->with_sets)
            eng.claims_match_set(V.arena, V.arena_len, jobs, n, exs.data(), (uint32_t)exs.size(), &match->paths,
                                 &match->preds, &match->args, &match->hargs, &match->sets, code, masks, true);
          else
            eng.claims_match_hash(V.arena, V.arena_len, jobs, n, exs.data(), (uint32_t)exs.size(), &match->paths,
                                  &match->preds, &match->args, &match->hargs, code, masks, true);
        } else if (match->with_args)
          eng.claims_match_args(V.arena, V.arena_len, jobs, n, exs.data(), (uint32_t)exs.size(), &match->paths,
                                &match->preds, &match->args, code, masks, true);
        else
          eng.claims_match(V.arena, V.arena_len, jobs, n, exs.data(), (uint32_t)exs.size(), &match->paths,
                           &match->preds, code, masks, true);
      } else if constexpr (M == kPathMode)
        eng.claims_paths(V.arena, V.arena_len, jobs, n, exs.data(), (uint32_t)exs.size(), paths, code, recs, sels, true);
      else if constexpr (Each)
        eng.claims_each(V.arena, V.arena_len, jobs, n, exs.data(), (uint32_t)exs.size(),
                        M == kSelectMode ? select : nullptr, code, X ? recs : nullptr,
                        M == kSelectMode ? sels : nullptr, true);
      else if constexpr (M == kSelectMode) eng.claims_select(V.arena, V.arena_len, jobs, n, &ex, select, code, recs, sels, true);
      else if constexpr (X) eng.claims_extract(V.arena, V.arena_len, jobs, n, &ex, code, recs, true);
      else eng.claims_scan(V.arena, V.arena_len, jobs, n, &ex, code, true);
    } catch (const DeviceError& e) {
      // as a failed verify: the tokens the scan carried get its error (no
      // host fallback for them) and the context is recreated after the batch
      scan_failed = true;
      scan_err = std::string("capjwt: claims scan unavailable: ") + e.what();
      scan_seen = eng.errors();
    }
    pt.lap("scan");
  };
  std::shared_ptr<Verified> V = ks_->verify_raw(tokens, &overlap);
  if (scan_failed) (void)eng.recover(scan_seen);
  PhaseTimer pt("check");
  const Chunks ch = make_chunks(n, th);
  std::vector<size_t> n_scan(ch.count(), 0), n_host(ch.count(), 0);
  // The host path of HashOfArg: one jg_hash_batch call over the values of just the tokens that take it.
  bool hash_failed = false;
  std::string hash_err;
  std::vector<uint8_t> needs_hash;
  if constexpr (M == kMatchMode) {
    if (match->with_hash && match->hash_reqs) {
      const size_t nh = match->hashes->size();
      std::vector<jg_hjob> hjobs;
      std::vector<size_t> at;                           // i * nh + c of each job
      std::string harena;
      for (size_t i = 0; i < n; ++i) {
        const Tok& t = V->toks[i];
        if (!(t.parsed && !V->failed[i] && V->any[i]) || code[i] != JG_CL_HOST) continue;
        if (scan_failed && have_jobs && jobs[i].len) continue;
        const int fam = hash_fam_of_alg(t.alg);
        for (size_t c = 0; c < nh && fam; ++c) {
          const auto& v = (*match->hashes)[c][i];
          if (!v) continue;
          jg_hjob j{};
          j.off = harena.size();
          j.len = (uint32_t)v->size();
          j.fam = (uint8_t)fam;
          hjobs.push_back(j);
          at.push_back(i * nh + c);
          harena.append(*v);
        }
      }
      if (!hjobs.empty()) {
        match->hosted.assign(n * nh, std::string());
        std::vector<uint8_t> dig(64 * hjobs.size());
        try {
          eng.hash((const uint8_t*)harena.data(), harena.size(), hjobs.data(), hjobs.size(), dig.data());
          for (size_t k = 0; k < hjobs.size(); ++k) match->hosted[at[k]] = hash_claim_value(&dig[64 * k], hjobs[k].fam);
        } catch (const DeviceError& e) {
          // as a failed scan: the tokens that needed the device get its error, and the context is recreated
          hash_failed = true;
          hash_err = std::string("capjwt: claims scan unavailable: ") + e.what();
          needs_hash.assign(n, 0);
          for (size_t k : at) needs_hash[k / nh] = 1;
          (void)eng.recover(eng.errors());
        }
      }
    }
  }
  const Expected* const one = exps;                   // Each = false: the one Expected and its clock
  const int64_t one_now = Each ? 0 : prof[0].now;
  run_chunks(ch, [&](size_t c, size_t lo, size_t hi) {
    size_t ns = 0, nh = 0;
    for (size_t i = lo; i < hi; ++i) {
      const Tok& t = V->toks[i];
      const Expected& expected = Each ? exps[which[i]] : *one;
      const int64_t now = Each ? prof[which[i]].now : one_now;
      if (!(t.parsed && !V->failed[i] && V->any[i])) {
        Result r;                                     // the key set's own error string; no claims are read
        ks_->finish(*V, i, r);
        reject(c, i, "error verifying token signature: " + r.err);
        continue;
      }
      if (scan_failed && have_jobs && jobs[i].len) {
        reject(c, i, std::string(scan_err));
        continue;
      }
      if (code[i] == JG_CL_HOST) {
        ++nh;
        if (hash_failed && needs_hash[i]) {
          reject(c, i, std::string(hash_err));
          continue;
        }
        Result r;
        ks_->finish(*V, i, r);
        if (!r.ok) {
          reject(c, i, "error verifying token signature: " + r.err);
          continue;
        }
        if constexpr (X) {
          RegisteredClaims rc;
          Result v = validate_claims(r.claims, t.view(), expected, now, &rc);
          if (!v.ok) reject(c, i, std::move(v.err));
          else if constexpr (M >= kSelectMode) put.claims(c, i, std::move(rc), r.claims);
          else put.claims(c, i, std::move(rc));
        } else {
          Result v = validate_claims(r.claims, t.view(), expected, now);
          if constexpr (M == kMatchMode) {
            const uint32_t bits = !v.ok ? 0u : match->with_args ? match->host_bits(r.claims, i)
                                                                : match_requires(r.claims, match->reqs);
            put(i, v.ok, std::move(v.err), bits);
          } else {
            put(i, v.ok, std::move(v.err));
          }
        }
        continue;
      }
      ++ns;
      std::string err = alg_header_error(t.view(), expected);
      if (!err.empty()) {
        reject(c, i, std::move(err));
        continue;
      }
      if constexpr (X) {
        // the payload segment ends the signing input; its length is the job's
        if (code[i] != JG_CL_OK) reject(c, i, std::string(claim_code_error(code[i])));
        else if constexpr (M >= kSelectMode)
          put.record(c, i, std::string_view(t.lit + t.si_len - jobs[i].len, jobs[i].len), recs[i], sels[i]);
        else
          put.record(c, i, std::string_view(t.lit + t.si_len - jobs[i].len, jobs[i].len), recs[i]);
      } else if constexpr (M == kMatchMode) {
        put(i, code[i] == JG_CL_OK, std::string(claim_code_error(code[i])),
            code[i] == JG_CL_OK ? match->spread(masks[i]) : 0u);
      } else {
        put(i, code[i] == JG_CL_OK, std::string(claim_code_error(code[i])));
      }
    }
    n_scan[c] = ns;
    n_host[c] = nh;
  });
  pt.lap("merge");
  if (stats) {
    stats->scanned = stats->host = 0;
    for (size_t c = 0; c < ch.count(); ++c) {
      stats->scanned += n_scan[c];
      stats->host += n_host[c];
    }
  }
  V->toks.release();
  pt.lap("free-toks");
}
}  // namespace

std::vector<CheckResult> Validator::CheckBatch(const std::vector<std::string_view>& tokens, const Expected& expected,
                                               CheckStats* stats) {
  std::vector<CheckResult> out(tokens.size());
  check_core<kCheckMode, false>(ks_, tokens, &expected, 1, nullptr, stats, [&](size_t i, bool ok, std::string&& err) {
    out[i].ok = ok;
    out[i].err = std::move(err);
  });
  return out;
}

namespace {
struct RowSink {                                   // RegisteredBatch: one RegisteredResult per token
  std::vector<RegisteredResult>& out;
  void reject(size_t, size_t i, std::string&& err) { out[i].err = std::move(err); }
  void record(size_t, size_t i, std::string_view seg, const jg_claims& v) {
    out[i].ok = true;
    out[i].claims = claims_of_record(seg, v);
  }
  void claims(size_t, size_t i, RegisteredClaims&& c) {
    out[i].ok = true;
    out[i].claims = std::move(c);
  }
};

// RegisteredCols: the fixed columns are written in place; each merge thread
// appends its chunk's bytes to a part of its own, with offsets relative to the
// part, and finish() moves the parts into the caller's memory
struct ColumnSink {
  struct Part {
    std::string str[3], aud;
    std::vector<uint32_t> aud_end;                 // each element's end in `aud`
    bool sized = false;
  };
  const RegisteredColumns& R;
  const Chunks& ch;
  std::vector<Part> parts;
  uint32_t* off[3];
  ColumnSink(const RegisteredColumns& r, const Chunks& chunks)
      : R(r), ch(chunks), parts(chunks.count()), off{r.iss_off, r.sub_off, r.jti_off} {}
  // The tokens of one batch mostly have one shape: the chunk's first record
  // sizes the part (a quarter over), so that it does not grow a dozen times
  // into fresh pages while 16 threads do the same.
  void size_part(Part& P, size_t c, const jg_claims& v) {
    P.sized = true;
    const size_t cnt = ch.b[c + 1] - ch.b[c];
    auto room = [&](uint32_t len) { return cnt * ((size_t)len + len / 4 + 4); };
    P.str[0].reserve(room(v.iss_len));
    P.str[1].reserve(room(v.sub_len));
    P.str[2].reserve(room(v.jti_len));
    P.aud.reserve(room(v.aud_len));
    P.aud_end.reserve(cnt * ((size_t)v.aud_n + 1));
  }
  void row(Part& P, size_t i, bool ok, uint32_t present, int64_t exp, int64_t nbf, int64_t iat) {
    R.ok[i] = ok ? 1 : 0;
    R.present[i] = (uint8_t)(present & 0xe0u);
    R.exp[i] = exp;
    R.nbf[i] = nbf;
    R.iat[i] = iat;
    for (int k = 0; k < 3; ++k) off[k][i + 1] = (uint32_t)P.str[k].size();
    R.aud_tok[i + 1] = (uint32_t)P.aud_end.size();
  }
  void reject(size_t c, size_t i, std::string&&) { row(parts[c], i, false, 0, 0, 0, 0); }
  void record(size_t c, size_t i, std::string_view seg, const jg_claims& v) {
    Part& P = parts[c];
    if (!P.sized) size_part(P, c, v);
    append_span(P.str[0], seg, v.iss_off, v.iss_len);
    append_span(P.str[1], seg, v.sub_off, v.sub_len);
    append_span(P.str[2], seg, v.jti_off, v.jti_len);
    if (v.aud_n) {
      // the value's text goes to the end of the part, its elements are moved down over it
      const size_t at = P.aud.size();
      append_span(P.aud, seg, v.aud_off, v.aud_len);
      size_t w = at;
      aud_elements(std::string_view(P.aud).substr(at), [&](size_t b, size_t n) {
        std::memmove(&P.aud[w], &P.aud[at + b], n);
        w += n;
        P.aud_end.push_back((uint32_t)w);
      });
      P.aud.resize(w);
    }
    row(P, i, true, v.present, v.exp, v.nbf, v.iat);
  }
  void claims(size_t c, size_t i, RegisteredClaims&& cl) {
    Part& P = parts[c];
    P.str[0] += cl.Issuer;
    P.str[1] += cl.Subject;
    P.str[2] += cl.ID;
    for (const auto& a : cl.Audience) {
      P.aud += a;
      P.aud_end.push_back((uint32_t)P.aud.size());
    }
    row(P, i, true, (cl.Expiry ? 1u << 5 : 0u) | (cl.NotBefore ? 1u << 6 : 0u) | (cl.IssuedAt ? 1u << 7 : 0u),
        cl.Expiry.value_or(0), cl.NotBefore.value_or(0), cl.IssuedAt.value_or(0));
  }
  void finish() {
    const size_t nc = parts.size();
    std::vector<size_t> base[4], ebase(nc + 1, 0);
    for (int k = 0; k < 4; ++k) {
      base[k].assign(nc + 1, 0);
      for (size_t c = 0; c < nc; ++c) base[k][c + 1] = base[k][c] + (k < 3 ? parts[c].str[k] : parts[c].aud).size();
    }
    for (size_t c = 0; c < nc; ++c) ebase[c + 1] = ebase[c] + parts[c].aud_end.size();
    char* data[4];
    for (int k = 0; k < 4; ++k) data[k] = (char*)R.alloc((RegisteredColumns::Var)k, base[k][nc]);
    uint32_t* const aud_off = (uint32_t*)R.alloc(RegisteredColumns::AUD_OFF, 4 * (ebase[nc] + 1));
    aud_off[0] = 0;
    for (int k = 0; k < 3; ++k) off[k][0] = 0;
    R.aud_tok[0] = 0;
    run_chunks(ch, [&](size_t c, size_t lo, size_t hi) {
      const Part& P = parts[c];
      for (int k = 0; k < 4; ++k) {
        const std::string& src = k < 3 ? P.str[k] : P.aud;
        if (!src.empty()) std::memcpy(data[k] + base[k][c], src.data(), src.size());
      }
      for (size_t i = lo; i < hi; ++i) {
        for (int k = 0; k < 3; ++k) off[k][i + 1] += (uint32_t)base[k][c];
        R.aud_tok[i + 1] += (uint32_t)ebase[c];
      }
      for (size_t j = 0; j < P.aud_end.size(); ++j) aud_off[ebase[c] + j + 1] = (uint32_t)(base[3][c] + P.aud_end[j]);
    });
  }
};
}  // namespace

std::vector<RegisteredResult> Validator::RegisteredBatch(const std::vector<std::string_view>& tokens,
                                                         const Expected& expected, CheckStats* stats) {
  std::vector<RegisteredResult> out(tokens.size());
  check_core<kRegisteredMode, false>(ks_, tokens, &expected, 1, nullptr, stats, RowSink{out});
  return out;
}

void Validator::RegisteredCols(const std::vector<std::string_view>& tokens, const Expected& expected,
                               const RegisteredColumns& out, CheckStats* stats) {
  const Chunks ch = make_chunks(tokens.size(), host_threads());      // check_core's own chunks
  ColumnSink sink(out, ch);
  check_core<kRegisteredMode, false>(ks_, tokens, &expected, 1, nullptr, stats, sink);
  PhaseTimer pt("check");
  sink.finish();
  pt.lap("columns");
}

namespace {
// The caller's names as the scan takes them (jg_select): equal names share a
// slot.  usable == false: the ABI does not take the list and every token goes
// the host path.
struct SelectNames {
  std::string bytes;
  jg_select abi{};
  std::vector<int> slot;                           // names[k] is slot[k] of a jg_selected
  bool usable = true;
  const std::vector<std::string>& names;
  size_t size() const { return names.size(); }
  // the entry of a host-path token's verified claims map
  const json::Value* find(const json::Value& all, size_t k) const { return all.get(names[k]); }
  explicit SelectNames(const std::vector<std::string>& names) : slot(names.size(), -1), names(names) {
    std::vector<std::string_view> uniq;
    for (size_t k = 0; k < names.size(); ++k) {
      const std::string& nm = names[k];
      if (nm.find('\0') != std::string::npos) throw std::invalid_argument("capjwt: a claim name holds a NUL byte");
      if (nm.empty() || nm.size() > JG_SELECT_NAME_MAX) usable = false;
      for (unsigned char c : nm)
        if (c < 0x20 || c > 0x7e || c == '"' || c == '\\') usable = false;
      size_t u = 0;
      while (u < uniq.size() && uniq[u] != nm) ++u;
      if (u == uniq.size()) uniq.push_back(nm);
      slot[k] = (int)u;
    }
    if (uniq.size() > JG_MAX_SELECT) usable = false;
    if (!usable) return;
    for (size_t u = 0; u < uniq.size(); ++u) {
      abi.name_len[u] = (uint32_t)uniq[u].size();
      bytes += uniq[u];
    }
    abi.n = (uint32_t)uniq.size();
    abi.names = (const uint8_t*)bytes.data();
  }
  const jg_select* select() const { return usable ? &abi : nullptr; }
};

// The caller's paths as the scan takes them (jg_paths), as SelectNames holds
// names: equal paths share a slot; usable == false: every token goes the host path.
struct SelectPaths {
  std::string bytes;
  jg_paths abi{};
  std::vector<int> slot;                           // paths[k] is slot[k] of a jg_selected
  bool usable = true;
  const std::vector<ClaimPath>& paths;
  size_t size() const { return paths.size(); }
  // the claims map walked along path k: every value on the way an object that holds the key
  const json::Value* find(const json::Value& all, size_t k) const {
    const json::Value* cur = &all;
    for (const std::string& comp : paths[k]) {
      if (cur->kind != json::Value::Object) return nullptr;
      cur = cur->get(comp);
      if (!cur) return nullptr;
    }
    return cur;
  }
  explicit SelectPaths(const std::vector<ClaimPath>& paths) : slot(paths.size(), -1), paths(paths) {
    std::vector<const ClaimPath*> uniq;
    for (size_t k = 0; k < paths.size(); ++k) {
      const ClaimPath& path = paths[k];
      if (path.empty()) throw std::invalid_argument("capjwt: a claim path has no component");
      if (path.size() > JG_PATH_MAX_COMP) usable = false;
      for (const std::string& comp : path) {
        if (comp.find('\0') != std::string::npos) throw std::invalid_argument("capjwt: a claim path holds a NUL byte");
        if (comp.empty() || comp.size() > JG_SELECT_NAME_MAX) usable = false;
        for (unsigned char c : comp)
          if (c < 0x20 || c > 0x7e || c == '"' || c == '\\') usable = false;
      }
      size_t u = 0;
      while (u < uniq.size() && *uniq[u] != path) ++u;
      if (u == uniq.size()) uniq.push_back(&path);
      slot[k] = (int)u;
    }
    if (uniq.size() > JG_MAX_PATHS) usable = false;
    if (!usable) return;
    for (size_t u = 0; u < uniq.size(); ++u) {
      abi.ncomp[u] = (uint32_t)uniq[u]->size();
      for (size_t d = 0; d < uniq[u]->size(); ++d) {
        abi.comp_len[u][d] = (uint32_t)(*uniq[u])[d].size();
        bytes += (*uniq[u])[d];
      }
    }
    abi.n = (uint32_t)uniq.size();
    abi.names = (const uint8_t*)bytes.data();
  }
  const jg_paths* select() const { return usable ? &abi : nullptr; }
};

// The claims-map entry a slot of the scan's record stands for.  A string whose
// bytes are ASCII is cut out of the decoded payload; a number, a string with
// bytes >= 0x80, an array or an object is parsed from its own span (the parser
// the claims map is read with, so numbers and invalid UTF-8 come out the same).
std::optional<json::Value> value_of_slot(std::string_view seg, const jg_selected& q, int slot) {
  std::optional<json::Value> out;
  const uint8_t type = q.type[slot];
  if (type == JG_SEL_ABSENT) return out;
  json::Value& v = out.emplace();
  std::string text;
  switch (type) {
    case JG_SEL_NULL: break;
    case JG_SEL_TRUE:
    case JG_SEL_FALSE:
      v.kind = json::Value::Bool;
      v.b = type == JG_SEL_TRUE;
      break;
    case JG_SEL_STRING:
      append_span(text, seg, q.off[slot], q.len[slot]);
      v.kind = json::Value::String;
      v.str = std::string_view(text);
      break;
    default: {
      append_span(text, seg, q.off[slot], q.len[slot]);
      std::string err;
      if (!json::parse(text, &v, &err)) throw std::logic_error("capjwt: the claims scan returned a span that does not parse: " + err);
    }
  }
  return out;
}

uint8_t sel_type_of(const json::Value& v) {
  switch (v.kind) {
    case json::Value::Null: return JG_SEL_NULL;
    case json::Value::Bool: return v.b ? JG_SEL_TRUE : JG_SEL_FALSE;
    case json::Value::Number: return JG_SEL_NUMBER;
    case json::Value::String: return JG_SEL_STRING;
    case json::Value::Array: return JG_SEL_ARRAY;
    default: return JG_SEL_OBJECT;
  }
}

template <class Keys>                              // SelectNames or SelectPaths
struct SelectRowSink {                             // SelectBatch: one SelectResult per token
  std::vector<SelectResult>& out;
  const Keys& N;
  void reject(size_t, size_t i, std::string&& err) { out[i].err = std::move(err); }
  void record(size_t, size_t i, std::string_view seg, const jg_claims& v, const jg_selected& q) {
    out[i].ok = true;
    out[i].claims = claims_of_record(seg, v);
    out[i].values.resize(N.size());
    for (size_t k = 0; k < N.size(); ++k) out[i].values[k] = value_of_slot(seg, q, N.slot[k]);
  }
  void claims(size_t, size_t i, RegisteredClaims&& c, const json::Value& all) {
    out[i].ok = true;
    out[i].claims = std::move(c);
    out[i].values.resize(N.size());
    for (size_t k = 0; k < N.size(); ++k)
      if (const json::Value* m = N.find(all, k)) out[i].values[k] = *m;
  }
};

// SelectCols: ColumnSink for the registered columns; per name the type and the
// number are written in place and the text goes to the merge thread's part
template <class Keys>
struct SelectColumnSink {
  ColumnSink reg;
  const SelectColumns& S;
  const Keys& N;
  const Chunks& ch;
  std::vector<std::vector<std::string>> text;      // [chunk][name]
  SelectColumnSink(const SelectColumns& s, const Keys& sn, const Chunks& chunks)
      : reg(s.reg, chunks), S(s), N(sn), ch(chunks), text(chunks.count(), std::vector<std::string>(sn.size())) {}
  void cell(size_t c, size_t i, size_t k, const json::Value* v, uint8_t type) {
    std::string& T = text[c][k];
    if (v) {
      if (v->kind == json::Value::String) T.append(v->str.data(), v->str.size());
      else if (v->kind == json::Value::Array || v->kind == json::Value::Object) T += json::marshal(*v);
    }
    S.names[k].type[i] = type;
    S.names[k].num[i] = v && v->kind == json::Value::Number ? v->num : 0.0;
    S.names[k].text_off[i + 1] = (uint32_t)T.size();
  }
  void reject(size_t c, size_t i, std::string&& err) {
    reg.reject(c, i, std::move(err));
    for (size_t k = 0; k < N.size(); ++k) cell(c, i, k, nullptr, JG_SEL_ABSENT);
  }
  void record(size_t c, size_t i, std::string_view seg, const jg_claims& v, const jg_selected& q) {
    reg.record(c, i, seg, v);
    for (size_t k = 0; k < N.size(); ++k) {
      const int slot = N.slot[k];
      if (q.type[slot] == JG_SEL_STRING) {         // the common case: straight from the payload into the part
        append_span(text[c][k], seg, q.off[slot], q.len[slot]);
        cell(c, i, k, nullptr, JG_SEL_STRING);
        continue;
      }
      const std::optional<json::Value> val = value_of_slot(seg, q, slot);
      cell(c, i, k, val ? &*val : nullptr, q.type[slot]);
    }
  }
  void claims(size_t c, size_t i, RegisteredClaims&& cl, const json::Value& all) {
    reg.claims(c, i, std::move(cl));
    for (size_t k = 0; k < N.size(); ++k) {
      const json::Value* m = N.find(all, k);
      cell(c, i, k, m, m ? sel_type_of(*m) : (uint8_t)JG_SEL_ABSENT);
    }
  }
  void finish() {
    reg.finish();
    const size_t nc = text.size();
    for (size_t k = 0; k < N.size(); ++k) {
      std::vector<size_t> base(nc + 1, 0);
      for (size_t c = 0; c < nc; ++c) base[c + 1] = base[c] + text[c][k].size();
      char* const data = (char*)S.alloc_text(k, base[nc]);
      uint32_t* const off = S.names[k].text_off;
      off[0] = 0;
      run_chunks(ch, [&](size_t c, size_t lo, size_t hi) {
        const std::string& src = text[c][k];
        if (!src.empty()) std::memcpy(data + base[c], src.data(), src.size());
        for (size_t i = lo; i < hi; ++i) off[i + 1] += (uint32_t)base[c];
      });
    }
  }
};
}  // namespace

std::vector<SelectResult> Validator::SelectBatch(const std::vector<std::string_view>& tokens, const Expected& expected,
                                                 const std::vector<std::string>& names, CheckStats* stats) {
  const SelectNames N(names);
  std::vector<SelectResult> out(tokens.size());
  check_core<kSelectMode, false>(ks_, tokens, &expected, 1, nullptr, stats, SelectRowSink<SelectNames>{out, N}, N.select());
  return out;
}

void Validator::SelectCols(const std::vector<std::string_view>& tokens, const Expected& expected,
                           const std::vector<std::string>& names, const SelectColumns& out, CheckStats* stats) {
  if (out.names.size() != names.size()) throw std::invalid_argument("capjwt: SelectCols: one column set per name");
  const SelectNames N(names);
  const Chunks ch = make_chunks(tokens.size(), host_threads());      // check_core's own chunks
  SelectColumnSink<SelectNames> sink(out, N, ch);
  check_core<kSelectMode, false>(ks_, tokens, &expected, 1, nullptr, stats, sink, N.select());
  PhaseTimer pt("check");
  sink.finish();
  pt.lap("columns");
}

std::vector<uint8_t> Validator::CheckVerdicts(const std::vector<std::string_view>& tokens, const Expected& expected,
                                              CheckStats* stats) {
  std::vector<uint8_t> ok(tokens.size(), 0);
  check_core<kCheckMode, false>(ks_, tokens, &expected, 1, nullptr, stats,
                                [&](size_t i, bool good, std::string&&) { ok[i] = good ? 1 : 0; });
  return ok;
}

// ---- the same six with an Expected per token
namespace {
void each_args(const char* what, const std::vector<std::string_view>& tokens, const std::vector<Expected>& expected,
               const std::vector<uint32_t>& which) {
  if (which.size() != tokens.size())
    throw std::invalid_argument(std::string("capjwt: ") + what + ": one profile index per token");
  if (expected.empty() && !tokens.empty())
    throw std::invalid_argument(std::string("capjwt: ") + what + ": no Expected");
  for (size_t i = 0; i < which.size(); ++i)
    if (which[i] >= expected.size())
      throw std::invalid_argument(std::string("capjwt: ") + what + ": token " + std::to_string(i) +
                                  " names profile " + std::to_string(which[i]) + " of " +
                                  std::to_string(expected.size()));
}
}  // namespace

std::vector<CheckResult> Validator::CheckBatchEach(const std::vector<std::string_view>& tokens,
                                                   const std::vector<Expected>& expected,
                                                   const std::vector<uint32_t>& which, CheckStats* stats) {
  each_args("CheckBatchEach", tokens, expected, which);
  std::vector<CheckResult> out(tokens.size());
  check_core<kCheckMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats,
                               [&](size_t i, bool ok, std::string&& err) {
                                 out[i].ok = ok;
                                 out[i].err = std::move(err);
                               });
  return out;
}

std::vector<uint8_t> Validator::CheckVerdictsEach(const std::vector<std::string_view>& tokens,
                                                  const std::vector<Expected>& expected,
                                                  const std::vector<uint32_t>& which, CheckStats* stats) {
  each_args("CheckVerdictsEach", tokens, expected, which);
  std::vector<uint8_t> ok(tokens.size(), 0);
  check_core<kCheckMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats,
                               [&](size_t i, bool good, std::string&&) { ok[i] = good ? 1 : 0; });
  return ok;
}

std::vector<RegisteredResult> Validator::RegisteredBatchEach(const std::vector<std::string_view>& tokens,
                                                             const std::vector<Expected>& expected,
                                                             const std::vector<uint32_t>& which, CheckStats* stats) {
  each_args("RegisteredBatchEach", tokens, expected, which);
  std::vector<RegisteredResult> out(tokens.size());
  check_core<kRegisteredMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats, RowSink{out});
  return out;
}

void Validator::RegisteredColsEach(const std::vector<std::string_view>& tokens, const std::vector<Expected>& expected,
                                   const std::vector<uint32_t>& which, const RegisteredColumns& out,
                                   CheckStats* stats) {
  each_args("RegisteredColsEach", tokens, expected, which);
  const Chunks ch = make_chunks(tokens.size(), host_threads());      // check_core's own chunks
  ColumnSink sink(out, ch);
  check_core<kRegisteredMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats, sink);
  PhaseTimer pt("check");
  sink.finish();
  pt.lap("columns");
}

std::vector<SelectResult> Validator::SelectBatchEach(const std::vector<std::string_view>& tokens,
                                                     const std::vector<Expected>& expected,
                                                     const std::vector<uint32_t>& which,
                                                     const std::vector<std::string>& names, CheckStats* stats) {
  each_args("SelectBatchEach", tokens, expected, which);
  const SelectNames N(names);
  std::vector<SelectResult> out(tokens.size());
  check_core<kSelectMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats,
                                SelectRowSink<SelectNames>{out, N}, N.select());
  return out;
}

void Validator::SelectColsEach(const std::vector<std::string_view>& tokens, const std::vector<Expected>& expected,
                               const std::vector<uint32_t>& which, const std::vector<std::string>& names,
                               const SelectColumns& out, CheckStats* stats) {
  if (out.names.size() != names.size()) throw std::invalid_argument("capjwt: SelectColsEach: one column set per name");
  each_args("SelectColsEach", tokens, expected, which);
  const SelectNames N(names);
  const Chunks ch = make_chunks(tokens.size(), host_threads());      // check_core's own chunks
  SelectColumnSink<SelectNames> sink(out, N, ch);
  check_core<kSelectMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats, sink, N.select());
  PhaseTimer pt("check");
  sink.finish();
  pt.lap("columns");
}

// ---- the four Select entries by path
std::vector<SelectResult> Validator::SelectBatch(const std::vector<std::string_view>& tokens, const Expected& expected,
                                                 const ClaimPaths& paths, CheckStats* stats) {
  const SelectPaths N(paths.paths);
  std::vector<SelectResult> out(tokens.size());
  check_core<kPathMode, false>(ks_, tokens, &expected, 1, nullptr, stats, SelectRowSink<SelectPaths>{out, N}, nullptr,
                               N.select());
  return out;
}

void Validator::SelectCols(const std::vector<std::string_view>& tokens, const Expected& expected,
                           const ClaimPaths& paths, const SelectColumns& out, CheckStats* stats) {
  if (out.names.size() != paths.paths.size()) throw std::invalid_argument("capjwt: SelectCols: one column set per path");
  const SelectPaths N(paths.paths);
  const Chunks ch = make_chunks(tokens.size(), host_threads());      // check_core's own chunks
  SelectColumnSink<SelectPaths> sink(out, N, ch);
  check_core<kPathMode, false>(ks_, tokens, &expected, 1, nullptr, stats, sink, nullptr, N.select());
  PhaseTimer pt("check");
  sink.finish();
  pt.lap("columns");
}

std::vector<SelectResult> Validator::SelectBatchEach(const std::vector<std::string_view>& tokens,
                                                     const std::vector<Expected>& expected,
                                                     const std::vector<uint32_t>& which,
                                                     const ClaimPaths& paths, CheckStats* stats) {
  each_args("SelectBatchEach", tokens, expected, which);
  const SelectPaths N(paths.paths);
  std::vector<SelectResult> out(tokens.size());
  check_core<kPathMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats,
                              SelectRowSink<SelectPaths>{out, N}, nullptr, N.select());
  return out;
}

void Validator::SelectColsEach(const std::vector<std::string_view>& tokens, const std::vector<Expected>& expected,
                               const std::vector<uint32_t>& which, const ClaimPaths& paths,
                               const SelectColumns& out, CheckStats* stats) {
  if (out.names.size() != paths.paths.size()) throw std::invalid_argument("capjwt: SelectColsEach: one column set per path");
  each_args("SelectColsEach", tokens, expected, which);
  const SelectPaths N(paths.paths);
  const Chunks ch = make_chunks(tokens.size(), host_threads());      // check_core's own chunks
  SelectColumnSink<SelectPaths> sink(out, N, ch);
  check_core<kPathMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats, sink, nullptr,
                              N.select());
  PhaseTimer pt("check");
  sink.finish();
  pt.lap("columns");
}

// ====================================================================== oidc hash claims
template <class F>
void Engine::abi_call(const char* name, bool present, bool inside_verify, F&& call) {
  const std::string entry = std::string("capjwt: ") + name;
  std::shared_lock<std::shared_mutex> life(life_, std::defer_lock);
  if (!inside_verify) life.lock();
  if (!ctx_) fail_device("capjwt: device lost: " + lost_);
  if (!present) fail_device(entry + ": not provided by the loaded verifier library");
  const int rc = call();
  if (rc == -1) throw std::logic_error(entry + " rejected the host's jobs: " + jg_last_error(ctx_));
  if (rc != 0) fail_device(entry + ": " + jg_last_error(ctx_));
}

void Engine::hash(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, uint8_t* digests) {
  abi_call("jg_hash_batch", true, false,
           [&] { return jg_hash_batch(ctx_, arena, arena_len, (const jg_hjob*)jobs, njobs, digests); });
}

// ---- MatchBatch: predicates on claims, answered by the scan ----
namespace {
// what MatchBatch refuses whatever path decides the tokens
void check_requires(const std::vector<Require>& reqs, Require::Op max_op = Require::Present) {
  if (reqs.size() > kMaxRequires) throw std::invalid_argument("capjwt: more than 16 requirements: the mask has no bit for them");
  for (const Require& r : reqs) {
    if (r.path.empty()) throw std::invalid_argument("capjwt: a claim path has no component");
    for (const std::string& comp : r.path)
      if (comp.find('\0') != std::string::npos) throw std::invalid_argument("capjwt: a claim path holds a NUL byte");
    if (r.value.find('\0') != std::string::npos) throw std::invalid_argument("capjwt: a required value holds a NUL byte");
    if (r.op < Require::Equals || r.op > max_op)
      throw std::invalid_argument("capjwt: an unknown requirement op");
  }
}
bool scan_byte_ok(unsigned char c) { return c >= 0x20 && c <= 0x7e && c != '"' && c != '\\'; }

// how a requirement's other side travels in jg_preds::values: the text, the column (one byte), or the bound
std::string pred_value(const Require& r, int set_index = 0) {
  switch (r.op) {
    case Require::InSet: case Require::AnyElementIn: return std::string(1, (char)set_index);
    case Require::Present: case Require::IsString: return std::string();
    case Require::EqualsArg: case Require::AtLeastArg: case Require::AtMostArg: case Require::HashOfArg:
      return std::string(1, (char)r.column);
    case Require::AtLeast: case Require::AtMost: {
      std::string v(8, '\0');
      for (int b = 0; b < 8; ++b) v[b] = (char)((uint64_t)r.bound >> (8 * b));
      return v;
    }
    default: return r.value;
  }
}

const std::vector<std::vector<std::string_view>> kNoStrs;
const std::vector<const int64_t*> kNoNums;
MatchPlan::MatchPlan(const std::vector<Require>& reqs) : MatchPlan(reqs, 0, kNoStrs, kNoNums, false) {}

MatchPlan::MatchPlan(const std::vector<Require>& reqs, size_t n, const std::vector<std::vector<std::string_view>>& strs_,
                     const std::vector<const int64_t*>& nums_, bool with_args_, const std::vector<HashColumn>* hashes_)
    : reqs(reqs), bit(reqs.size(), -1), with_args(with_args_), strs(&strs_), nums(&nums_), hashes(hashes_) {
  const bool plain = !with_args;                      // MatchBatch's rules: ops 1..4 only
  check_requires(reqs, plain ? Require::Present : Require::AnyElementIn);
  // the sets: a handle per set requirement, the distinct ones in order of first use are the call's indices
  std::vector<int> set_index(reqs.size(), 0);
  snaps.resize(reqs.size());
  for (size_t k = 0; k < reqs.size(); ++k) {
    const Require& r = reqs[k];
    if (r.op < Require::InSet) continue;
    if (!r.set.impl) throw std::invalid_argument("capjwt: an InSet or AnyElementIn requirement without a claim set");
    with_sets = true;
    size_t x = 0;
    while (x < set_impls.size() && set_impls[x] != r.set.impl) ++x;
    if (x == set_impls.size()) set_impls.push_back(r.set.impl);
    set_index[k] = (int)x;
    std::lock_guard<std::mutex> g(r.set.impl->mu);
    if (r.set.impl->closed) throw std::invalid_argument("capjwt: the claim set is closed");
    snaps[k] = r.set.impl->host;
    if (r.set.impl->host_only) usable = false;
  }
  if (set_impls.size() > JG_MAX_SETS) usable = false;
  if (usable)
    for (size_t x = 0; x < set_impls.size(); ++x) sets.id[x] = (uint32_t)set_impls[x]->id;
  sets.nsets = usable ? (uint32_t)set_impls.size() : 0u;
  const size_t nh = hashes ? hashes->size() : 0;
  with_hash = nh > 0;
  for (const Require& r : reqs) {
    if (r.op == Require::HashOfArg && r.column >= nh)
      throw std::invalid_argument("capjwt: a requirement names a hash column that was not given");
    with_hash = with_hash || r.op >= Require::HashOfArg;
    hash_reqs = hash_reqs || r.op == Require::HashOfArg;
  }
  for (size_t c = 0; c < nh; ++c)
    if ((*hashes)[c].size() != n) throw std::invalid_argument("capjwt: a hash column does not hold one entry per token");
  if (nh > JG_MAX_HASH_ARGS || strs_.size() + nh > JG_MAX_ARGS) usable = false;
  for (const Require& r : reqs) {
    if (r.op == Require::EqualsArg && r.column >= strs_.size())
      throw std::invalid_argument("capjwt: a requirement names a string column that was not given");
    if ((r.op == Require::AtLeastArg || r.op == Require::AtMostArg) && r.column >= nums_.size())
      throw std::invalid_argument("capjwt: a requirement names a number column that was not given");
  }
  for (const auto& col : strs_) {
    if (col.size() != n) throw std::invalid_argument("capjwt: a string column does not hold one operand per token");
  }
  for (const int64_t* col : nums_)
    if (!col && n) throw std::invalid_argument("capjwt: a number column does not hold one operand per token");
  if (strs_.size() > JG_MAX_ARGS || nums_.size() > JG_MAX_ARGS) usable = false;
  std::vector<const ClaimPath*> upaths;
  std::vector<size_t> upreds;                        // the first requirement of each distinct one
  std::vector<int> path_of(reqs.size(), -1);
  for (size_t k = 0; k < reqs.size(); ++k) {
    const Require& r = reqs[k];
    if (r.path.size() > JG_PATH_MAX_COMP) usable = false;
    for (const std::string& comp : r.path) {
      if (comp.empty() || comp.size() > JG_SELECT_NAME_MAX) usable = false;
      for (unsigned char c : comp)
        if (!scan_byte_ok(c)) usable = false;
    }
    // Present ignores its value on both paths; an operand or a bound is no text
    const size_t vlen = r.op >= Require::Present ? 0 : r.value.size();
    if (vlen > JG_PRED_VALUE_MAX) usable = false;
    if ((r.op == Require::HasWord || r.op == Require::HasElement) && vlen == 0) usable = false;
    for (size_t b = 0; b < vlen; ++b)
      if (!scan_byte_ok((unsigned char)r.value[b]) || (r.op == Require::HasWord && r.value[b] == ' ')) usable = false;
    size_t u = 0;
    while (u < upaths.size() && *upaths[u] != r.path) ++u;
    if (u == upaths.size()) upaths.push_back(&r.path);
    path_of[k] = (int)u;
    size_t q = 0;
    for (; q < upreds.size(); ++q) {
      const Require& o = reqs[upreds[q]];
      if (path_of[upreds[q]] == path_of[k] && o.op == r.op &&
          pred_value(o, set_index[upreds[q]]) == pred_value(r, set_index[k]))
        break;
    }
    if (q == upreds.size()) upreds.push_back(k);
    bit[k] = (int)q;
    identity = identity && q == k;
  }
  if (upaths.size() > JG_MAX_PATHS) usable = false;
  if (!usable) {                                     // every token takes the host path; a NUL still throws
    for (const auto& col : strs_)
      for (const std::string_view v : col)
        if (v.find('\0') != std::string_view::npos) throw std::invalid_argument("capjwt: an operand holds a NUL byte");
    return;
  }
  for (size_t u = 0; u < upaths.size(); ++u) {
    paths.ncomp[u] = (uint32_t)upaths[u]->size();
    for (size_t d = 0; d < upaths[u]->size(); ++d) {
      paths.comp_len[u][d] = (uint32_t)(*upaths[u])[d].size();
      names += (*upaths[u])[d];
    }
  }
  paths.n = (uint32_t)upaths.size();
  paths.names = (const uint8_t*)names.data();
  for (size_t q = 0; q < upreds.size(); ++q) {
    const Require& r = reqs[upreds[q]];
    preds.path[q] = (uint8_t)path_of[upreds[q]];
    preds.op[q] = (uint8_t)r.op;
    const std::string v = pred_value(r, set_index[upreds[q]]);
    preds.value_len[q] = (uint32_t)v.size();
    values += v;
  }
  preds.n = (uint32_t)upreds.size();
  preds.values = (const uint8_t*)values.data();
  if (plain) return;
  // the operands, job-major; a token with an operand the scan refuses keeps empty spans and is not scanned
  const size_t ns = strs_.size(), nn = nums_.size();
  host_only.assign(n, 0);
  aspans.assign(n * ns, jg_sarg{0, 0});
  anums.resize(n * nn);
  // count, prefix, fill over fixed ranges: a range's operands lie back to back from the range's own offset
  const Chunks ch = make_chunks(n, host_threads());
  std::vector<size_t> base(ch.count() + 1, 0);
  std::atomic<bool> nul{false};
  run_chunks(ch, [&](size_t c, size_t lo, size_t hi) {
    size_t bytes = 0;
    for (size_t i = lo; i < hi; ++i) {
      bool ok = true;
      size_t mine = 0;
      for (size_t k = 0; k < ns; ++k) {
        const std::string_view v = strs_[k][i];
        if (v.find('\0') != std::string_view::npos) nul.store(true, std::memory_order_relaxed);
        ok = ok && v.size() <= JG_PRED_VALUE_MAX;
        for (size_t b = 0; ok && b < v.size(); ++b) ok = scan_byte_ok((unsigned char)v[b]);
        mine += v.size();
      }
      host_only[i] = ok ? 0 : 1;
      bytes += ok ? mine : 0;
    }
    base[c + 1] = bytes;
  });
  if (nul.load()) throw std::invalid_argument("capjwt: an operand holds a NUL byte");
  for (size_t c = 0; c < ch.count(); ++c) base[c + 1] += base[c];
  if (base[ch.count()] > 0xffffffffu) {               // the spans are 32 bits
    usable = false;
    return;
  }
  abytes.resize(base[ch.count()]);
  run_chunks(ch, [&](size_t c, size_t lo, size_t hi) {
    size_t o = base[c];
    for (size_t i = lo; i < hi; ++i) {
      for (size_t k = 0; k < ns && !host_only[i]; ++k) {
        const std::string_view v = strs_[k][i];
        aspans[i * ns + k] = jg_sarg{(uint32_t)o, (uint32_t)v.size()};
        std::memcpy(&abytes[o], v.data(), v.size());
        o += v.size();
      }
      for (size_t k = 0; k < nn; ++k) anums[i * nn + k] = nums_[k][i];
    }
  });
  args.bytes = (const uint8_t*)abytes.data();
  args.bytes_len = abytes.size();
  args.str = aspans.data();
  args.num = anums.data();
  args.nstr = (uint32_t)ns;
  args.nnum = (uint32_t)nn;
  if (!nh) return;
  // the values to hash, job-major and back to back; the families are set when the tokens' algs are known
  hsrc.assign(n * nh, jg_hsrc{});
  size_t total = 0;
  for (size_t i = 0; i < n; ++i)
    for (size_t c = 0; c < nh; ++c) {
      const auto& v = (*hashes)[c][i];
      if (v && v->size() > JG_HASH_SRC_MAX) host_only[i] = 1;
    }
  for (size_t i = 0; i < n; ++i)
    for (size_t c = 0; c < nh && !host_only[i]; ++c)
      if ((*hashes)[c][i]) total += (*hashes)[c][i]->size();
  if (total > 0xffffffffu - 4096) {
    usable = false;
    return;
  }
  hbytes.resize(total);
  size_t o = 0;
  for (size_t i = 0; i < n; ++i)
    for (size_t c = 0; c < nh && !host_only[i]; ++c) {
      const auto& v = (*hashes)[c][i];
      if (!v) continue;
      hsrc[i * nh + c].off = (uint32_t)o;
      hsrc[i * nh + c].len = (uint32_t)v->size();
      hsrc[i * nh + c].fam = 0xff;                      // a value: set_families() puts the token's family here
      if (!v->empty()) std::memcpy(&hbytes[o], v->data(), v->size());
      o += v->size();
    }
  hargs.bytes = (const uint8_t*)hbytes.data();
  hargs.bytes_len = hbytes.size();
  hargs.src = hsrc.data();
  hargs.nhash = (uint32_t)nh;
}

// the SHA-2 of an id_token's hash claims by its alg (oidc/id_token.go:106-119); 0: none (EdDSA, no alg)
int hash_fam_of_alg(int alg) {
  switch (alg) {
    case JG_RS256: case JG_ES256: case JG_PS256: return JG_SHA256;
    case JG_RS384: case JG_ES384: case JG_PS384: return JG_SHA384;
    case JG_RS512: case JG_ES512: case JG_PS512: return JG_SHA512;
    default: return 0;
  }
}
}  // namespace

std::string hash_claim_value(const uint8_t* digest, int fam) {
  const size_t half = (fam == JG_SHA256 ? 32 : fam == JG_SHA384 ? 48 : 64) / 2;
  return b64url_encode(std::string_view((const char*)digest, half));
}

namespace {
// the requirements on a claims map; strs / nums: one token's operands, for the ops that take one
// hashed: what the token's claim must equal under each hash column, "" for none
// snaps: per requirement the host copy of its set (InSet, AnyElementIn)
uint32_t requires_on(const json::Value& all_claims, const std::vector<Require>& reqs, const std::string_view* strs,
                     const int64_t* nums, const std::string* hashed = nullptr,
                     const std::shared_ptr<const HostSet>* snaps = nullptr) {
  uint32_t bits = 0;
  for (size_t k = 0; k < reqs.size(); ++k) {
    const Require& r = reqs[k];
    // the claims map walked along the path: every value on the way an object that holds the key
    const json::Value* v = &all_claims;
    for (const std::string& comp : r.path) {
      if (v->kind != json::Value::Object) { v = nullptr; break; }
      v = v->get(comp);
      if (!v) break;
    }
    if (!v) continue;
    bool hit = false;
    switch (r.op) {
      case Require::Present: hit = true; break;
      case Require::Equals: hit = v->kind == json::Value::String && v->str.view() == r.value; break;
      case Require::HasWord:
        if (v->kind == json::Value::String) {        // strings.Split(v, " "): only 0x20 separates, empty pieces count
          const std::string_view s = v->str.view();
          size_t at = 0;
          for (;;) {
            const size_t sp = s.find(' ', at);
            const std::string_view piece = s.substr(at, sp == std::string_view::npos ? std::string_view::npos : sp - at);
            if (piece == r.value) { hit = true; break; }
            if (sp == std::string_view::npos) break;
            at = sp + 1;
          }
        }
        break;
      case Require::HasElement:
        if (v->kind == json::Value::Array)
          for (const json::Value& e : v->arr)
            if (e.kind == json::Value::String && e.str.view() == r.value) { hit = true; break; }
        break;
      case Require::EqualsArg: hit = v->kind == json::Value::String && v->str.view() == strs[r.column]; break;
      // f, ok := v.(float64); ok && f >= float64(B)
      case Require::AtLeast: hit = v->kind == json::Value::Number && v->num >= (double)r.bound; break;
      case Require::AtMost: hit = v->kind == json::Value::Number && v->num <= (double)r.bound; break;
      case Require::AtLeastArg: hit = v->kind == json::Value::Number && v->num >= (double)nums[r.column]; break;
      case Require::AtMostArg: hit = v->kind == json::Value::Number && v->num <= (double)nums[r.column]; break;
      case Require::HashOfArg:
        hit = hashed && !hashed[r.column].empty() && v->kind == json::Value::String && v->str.view() == hashed[r.column];
        break;
      case Require::IsString: hit = v->kind == json::Value::String; break;
      // s, ok := v.(string); ok && set[s]
      case Require::InSet:
        hit = snaps && snaps[k] && v->kind == json::Value::String && snaps[k]->count(std::string(v->str.view())) != 0;
        break;
      case Require::AnyElementIn:
        if (snaps && snaps[k] && v->kind == json::Value::Array)
          for (const json::Value& e : v->arr)
            if (e.kind == json::Value::String && snaps[k]->count(std::string(e.str.view())) != 0) { hit = true; break; }
        break;
    }
    if (hit) bits |= 1u << k;
  }
  return bits;
}

uint32_t MatchPlan::host_bits(const json::Value& claims, size_t i) const {
  std::string_view s[JG_MAX_ARGS * 4];               // a list over the caps may hold more columns than the scan takes
  int64_t v[JG_MAX_ARGS * 4];
  const std::string* hx = hosted.empty() ? nullptr : &hosted[i * hashes->size()];
  if (strs->size() > JG_MAX_ARGS * 4 || nums->size() > JG_MAX_ARGS * 4) {
    std::vector<std::string_view> sv(strs->size());
    std::vector<int64_t> nv(nums->size());
    for (size_t c = 0; c < sv.size(); ++c) sv[c] = (*strs)[c][i];
    for (size_t c = 0; c < nv.size(); ++c) nv[c] = (*nums)[c][i];
    return requires_on(claims, reqs, sv.data(), nv.data(), hx, snaps.data());
  }
  for (size_t c = 0; c < strs->size(); ++c) s[c] = (*strs)[c][i];
  for (size_t c = 0; c < nums->size(); ++c) v[c] = (*nums)[c][i];
  return requires_on(claims, reqs, s, v, hx, snaps.data());
}
}  // namespace

uint32_t match_requires(const json::Value& all_claims, const std::vector<Require>& reqs) {
  check_requires(reqs);
  return requires_on(all_claims, reqs, nullptr, nullptr);
}

uint32_t match_requires(const json::Value& all_claims, const std::vector<Require>& reqs,
                        const std::vector<std::string_view>& strs, const std::vector<int64_t>& nums) {
  check_requires(reqs, Require::AtMostArg);
  for (const Require& r : reqs) {
    if (r.op == Require::EqualsArg && r.column >= strs.size())
      throw std::invalid_argument("capjwt: a requirement names a string column that was not given");
    if ((r.op == Require::AtLeastArg || r.op == Require::AtMostArg) && r.column >= nums.size())
      throw std::invalid_argument("capjwt: a requirement names a number column that was not given");
  }
  return requires_on(all_claims, reqs, strs.data(), nums.data());
}

uint32_t match_requires(const json::Value& all_claims, const std::vector<Require>& reqs,
                        const std::vector<std::string_view>& strs, const std::vector<int64_t>& nums,
                        const std::vector<std::optional<std::string>>& hashed) {
  check_requires(reqs, Require::AnyElementIn);
  std::vector<std::shared_ptr<const HostSet>> snaps(reqs.size());
  for (size_t k = 0; k < reqs.size(); ++k) {
    const Require& r = reqs[k];
    if (r.op == Require::EqualsArg && r.column >= strs.size())
      throw std::invalid_argument("capjwt: a requirement names a string column that was not given");
    if ((r.op == Require::AtLeastArg || r.op == Require::AtMostArg) && r.column >= nums.size())
      throw std::invalid_argument("capjwt: a requirement names a number column that was not given");
    if (r.op == Require::HashOfArg && r.column >= hashed.size())
      throw std::invalid_argument("capjwt: a requirement names a hash column that was not given");
    if (r.op >= Require::InSet) {
      if (!r.set.impl) throw std::invalid_argument("capjwt: an InSet or AnyElementIn requirement without a claim set");
      std::lock_guard<std::mutex> g(r.set.impl->mu);
      snaps[k] = r.set.impl->host;
    }
  }
  std::vector<std::string> hx(hashed.size());
  for (size_t c = 0; c < hashed.size(); ++c) hx[c] = hashed[c] ? *hashed[c] : std::string();
  return requires_on(all_claims, reqs, strs.data(), nums.data(), hx.data(), snaps.data());
}

std::vector<MatchResult> Validator::MatchBatch(const std::vector<std::string_view>& tokens, const Expected& expected,
                                               const std::vector<Require>& requires_, CheckStats* stats) {
  const MatchPlan plan(requires_);
  std::vector<MatchResult> out(tokens.size());
  check_core<kMatchMode, false>(ks_, tokens, &expected, 1, nullptr, stats,
                                [&](size_t i, bool ok, std::string&& err, uint32_t bits) {
                                  out[i].ok = ok;
                                  out[i].err = std::move(err);
                                  out[i].bits = bits;
                                }, nullptr, nullptr, &plan);
  return out;
}

void Validator::MatchVerdicts(const std::vector<std::string_view>& tokens, const Expected& expected,
                              const std::vector<Require>& requires_, uint8_t* ok_out, uint32_t* bits_out,
                              CheckStats* stats) {
  const MatchPlan plan(requires_);
  check_core<kMatchMode, false>(ks_, tokens, &expected, 1, nullptr, stats,
                                [&](size_t i, bool ok, std::string&&, uint32_t bits) {
                                  ok_out[i] = ok ? 1 : 0;
                                  bits_out[i] = bits;
                                }, nullptr, nullptr, &plan);
}

std::vector<MatchResult> Validator::MatchBatchEach(const std::vector<std::string_view>& tokens,
                                                   const std::vector<Expected>& expected,
                                                   const std::vector<uint32_t>& which,
                                                   const std::vector<Require>& requires_, CheckStats* stats) {
  each_args("MatchBatchEach", tokens, expected, which);
  const MatchPlan plan(requires_);
  std::vector<MatchResult> out(tokens.size());
  check_core<kMatchMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats,
                               [&](size_t i, bool ok, std::string&& err, uint32_t bits) {
                                 out[i].ok = ok;
                                 out[i].err = std::move(err);
                                 out[i].bits = bits;
                               }, nullptr, nullptr, &plan);
  return out;
}

void Validator::MatchVerdictsEach(const std::vector<std::string_view>& tokens, const std::vector<Expected>& expected,
                                  const std::vector<uint32_t>& which, const std::vector<Require>& requires_,
                                  uint8_t* ok_out, uint32_t* bits_out, CheckStats* stats) {
  each_args("MatchVerdictsEach", tokens, expected, which);
  const MatchPlan plan(requires_);
  check_core<kMatchMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats,
                               [&](size_t i, bool ok, std::string&&, uint32_t bits) {
                                 ok_out[i] = ok ? 1 : 0;
                                 bits_out[i] = bits;
                               }, nullptr, nullptr, &plan);
}

std::vector<MatchResult> Validator::MatchBatchArgs(const std::vector<std::string_view>& tokens, const Expected& expected,
                                                   const std::vector<Require>& requires_,
                                                   const std::vector<std::vector<std::string_view>>& strs,
                                                   const std::vector<const int64_t*>& nums, CheckStats* stats,
                                                   const std::vector<HashColumn>& hashes) {
  const MatchPlan plan(requires_, tokens.size(), strs, nums, true, &hashes);
  std::vector<MatchResult> out(tokens.size());
  check_core<kMatchMode, false>(ks_, tokens, &expected, 1, nullptr, stats,
                                [&](size_t i, bool ok, std::string&& err, uint32_t bits) {
                                  out[i].ok = ok;
                                  out[i].err = std::move(err);
                                  out[i].bits = bits;
                                }, nullptr, nullptr, &plan);
  return out;
}

void Validator::MatchVerdictsArgs(const std::vector<std::string_view>& tokens, const Expected& expected,
                                  const std::vector<Require>& requires_,
                                  const std::vector<std::vector<std::string_view>>& strs,
                                  const std::vector<const int64_t*>& nums, uint8_t* ok_out, uint32_t* bits_out,
                                  CheckStats* stats, const std::vector<HashColumn>& hashes) {
  const MatchPlan plan(requires_, tokens.size(), strs, nums, true, &hashes);
  check_core<kMatchMode, false>(ks_, tokens, &expected, 1, nullptr, stats,
                                [&](size_t i, bool ok, std::string&&, uint32_t bits) {
                                  ok_out[i] = ok ? 1 : 0;
                                  bits_out[i] = bits;
                                }, nullptr, nullptr, &plan);
}

std::vector<MatchResult> Validator::MatchBatchArgsEach(const std::vector<std::string_view>& tokens,
                                                       const std::vector<Expected>& expected,
                                                       const std::vector<uint32_t>& which,
                                                       const std::vector<Require>& requires_,
                                                       const std::vector<std::vector<std::string_view>>& strs,
                                                       const std::vector<const int64_t*>& nums, CheckStats* stats,
                                                       const std::vector<HashColumn>& hashes) {
  each_args("MatchBatchArgsEach", tokens, expected, which);
  const MatchPlan plan(requires_, tokens.size(), strs, nums, true, &hashes);
  std::vector<MatchResult> out(tokens.size());
  check_core<kMatchMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats,
                               [&](size_t i, bool ok, std::string&& err, uint32_t bits) {
                                 out[i].ok = ok;
                                 out[i].err = std::move(err);
                                 out[i].bits = bits;
                               }, nullptr, nullptr, &plan);
  return out;
}

void Validator::MatchVerdictsArgsEach(const std::vector<std::string_view>& tokens, const std::vector<Expected>& expected,
                                      const std::vector<uint32_t>& which, const std::vector<Require>& requires_,
                                      const std::vector<std::vector<std::string_view>>& strs,
                                      const std::vector<const int64_t*>& nums, uint8_t* ok_out, uint32_t* bits_out,
                                      CheckStats* stats, const std::vector<HashColumn>& hashes) {
  each_args("MatchVerdictsArgsEach", tokens, expected, which);
  const MatchPlan plan(requires_, tokens.size(), strs, nums, true, &hashes);
  check_core<kMatchMode, true>(ks_, tokens, expected.data(), expected.size(), which.data(), stats,
                               [&](size_t i, bool ok, std::string&&, uint32_t bits) {
                                 ok_out[i] = ok ? 1 : 0;
                                 bits_out[i] = bits;
                               }, nullptr, nullptr, &plan);
}

// The claims entries are the ones the host layer binds weakly: an ABI provider
// without them (the stub ABI the CPU unit tests link, an older libcapjwt.so)
// still links, and a CheckBatch against it reports the scan as unavailable, as
// any other device failure.  jg_claims_scan (CheckBatch), jg_claims_extract
// (RegisteredBatch), jg_claims_select (SelectBatch), jg_claims_each (the *Each
// entries: the three scans with a profile per job), jg_claims_paths (the
// Select entries by path), jg_claims_match (the Match entries),
// jg_claims_match_args (the MatchArgs entries) and jg_claims_match_hash (the
// MatchArgs entries with a hash column, HashOfArg or IsString).
extern "C" {
__attribute__((weak)) int jg_claims_scan(jg_ctx*, const uint8_t*, size_t, const jg_cjob*, size_t, const jg_expect*,
                                         uint8_t*);
__attribute__((weak)) int jg_claims_extract(jg_ctx*, const uint8_t*, size_t, const jg_cjob*, size_t, const jg_expect*,
                                            uint8_t*, jg_claims*);
__attribute__((weak)) int jg_claims_select(jg_ctx*, const uint8_t*, size_t, const jg_cjob*, size_t, const jg_expect*,
                                           const jg_select*, uint8_t*, jg_claims*, jg_selected*);
__attribute__((weak)) int jg_claims_each(jg_ctx*, const uint8_t*, size_t, const jg_cjob*, size_t, const jg_expect*,
                                         uint32_t, const jg_select*, uint8_t*, jg_claims*, jg_selected*);
__attribute__((weak)) int jg_claims_paths(jg_ctx*, const uint8_t*, size_t, const jg_cjob*, size_t, const jg_expect*,
                                          uint32_t, const jg_paths*, uint8_t*, jg_claims*, jg_selected*);
__attribute__((weak)) int jg_claims_match(jg_ctx*, const uint8_t*, size_t, const jg_cjob*, size_t, const jg_expect*,
                                          uint32_t, const jg_paths*, const jg_preds*, uint8_t*, uint32_t*);
__attribute__((weak)) int jg_claims_match_args(jg_ctx*, const uint8_t*, size_t, const jg_cjob*, size_t, const jg_expect*,
                                               uint32_t, const jg_paths*, const jg_preds*, const jg_args*, uint8_t*,
                                               uint32_t*);
__attribute__((weak)) int jg_claims_match_hash(jg_ctx*, const uint8_t*, size_t, const jg_cjob*, size_t, const jg_expect*,
                                               uint32_t, const jg_paths*, const jg_preds*, const jg_args*, const jg_hargs*,
                                               uint8_t*, uint32_t*);
// ... and the resident sets with their scan (the MatchArgs entries with InSet or AnyElementIn)
__attribute__((weak)) int jg_claims_match_set(jg_ctx*, const uint8_t*, size_t, const jg_cjob*, size_t, const jg_expect*,
                                              uint32_t, const jg_paths*, const jg_preds*, const jg_args*, const jg_hargs*,
                                              const jg_setargs*, uint8_t*, uint32_t*);
__attribute__((weak)) int jg_set_load(jg_ctx*, uint32_t, const uint8_t*, size_t, const jg_sarg*, size_t, uint32_t);
__attribute__((weak)) int jg_set_add(jg_ctx*, uint32_t, const uint8_t*, size_t, const jg_sarg*, size_t, uint32_t*);
__attribute__((weak)) int jg_set_free(jg_ctx*, uint32_t);
__attribute__((weak)) int jg_set_info(jg_ctx*, uint32_t, jg_setinfo*);
}

void Engine::claims_match_set(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs,
                              const void* expects, uint32_t nexpect, const void* paths, const void* preds,
                              const void* args, const void* hargs, const void* sets, uint8_t* codes, uint32_t* masks,
                              bool inside_verify) {
  abi_call("jg_claims_match_set", jg_claims_match_set != nullptr, inside_verify, [&] {
    return jg_claims_match_set(ctx_, arena, arena_len, (const jg_cjob*)jobs, njobs, (const jg_expect*)expects, nexpect,
                               (const jg_paths*)paths, (const jg_preds*)preds, (const jg_args*)args,
                               (const jg_hargs*)hargs, (const jg_setargs*)sets, codes, masks);
  });
}

// ---- resident sets ----
int Engine::set_acquire() {
  std::lock_guard<std::mutex> g(set_mu_);
  for (int id = 0; id < 16; ++id)
    if (!sets_[id].live) {
      sets_[id] = SetRecord{};
      sets_[id].live = true;
      return id;
    }
  throw std::runtime_error("capjwt: 16 claim sets are live on this key set: close one first");
}

// with set_mu_ held and ctx_ valid; a library without jg_set_load keeps the record only: its scan entry is
// missing too, and a call that names the set reports the scan as unavailable
int Engine::set_load_locked(int id) {
  if (!jg_set_load) return 0;
  const SetRecord& r = sets_[id];
  std::vector<jg_sarg> m(r.spans.size());
  for (size_t k = 0; k < m.size(); ++k) m[k] = jg_sarg{r.spans[k].first, r.spans[k].second};
  return jg_set_load(ctx_, (uint32_t)id, (const uint8_t*)r.bytes.data(), r.bytes.size(), m.data(), m.size(), r.seed);
}

void Engine::set_store(int id, const std::vector<std::string>& members, uint32_t seed) {
  SetRecord n;
  n.live = n.stored = true;
  n.seed = seed;
  for (const std::string& m : members) {
    n.spans.emplace_back((uint32_t)n.bytes.size(), (uint32_t)m.size());
    n.bytes += m;
  }
  std::shared_lock<std::shared_mutex> life(life_);
  std::lock_guard<std::mutex> g(set_mu_);
  if (!ctx_) throw std::runtime_error("capjwt: claim set not loaded: device lost: " + lost_);
  std::swap(sets_[id], n);
  const int rc = set_load_locked(id);
  if (rc != 0) {
    std::swap(sets_[id], n);                          // what the id held before stays in force, here as on the device
    throw std::runtime_error(std::string("capjwt: jg_set_load: ") + jg_last_error(ctx_));
  }
}

void Engine::set_add(int id, const std::vector<std::string>& members) {
  if (members.empty()) return;
  std::shared_lock<std::shared_mutex> life(life_);
  std::lock_guard<std::mutex> g(set_mu_);
  if (!ctx_) throw std::runtime_error("capjwt: claim set not added to: device lost: " + lost_);
  SetRecord& r = sets_[id];
  if (!r.live || !r.stored) throw std::runtime_error("capjwt: claim set not added to: the id holds no set");
  const size_t nbytes = r.bytes.size(), nspans = r.spans.size();
  for (const std::string& m : members) {
    r.spans.emplace_back((uint32_t)r.bytes.size(), (uint32_t)m.size());
    r.bytes += m;
  }
  int rc = 0;
  const char* entry = "jg_set_add";
  if (jg_set_add) {
    std::vector<jg_sarg> m(members.size());
    for (size_t k = 0; k < m.size(); ++k) m[k] = jg_sarg{r.spans[nspans + k].first, r.spans[nspans + k].second};
    rc = jg_set_add(ctx_, (uint32_t)id, (const uint8_t*)r.bytes.data(), r.bytes.size(), m.data(), m.size(), nullptr);
  } else {                                            // an older library: the union loaded whole, the same set
    entry = "jg_set_load";
    rc = set_load_locked(id);
  }
  if (rc != 0) {
    r.bytes.resize(nbytes);                           // what the id held before stays in force, here as on the device
    r.spans.resize(nspans);
    throw std::runtime_error(std::string("capjwt: ") + entry + ": " + jg_last_error(ctx_));
  }
}

void Engine::set_release(int id) {
  std::shared_lock<std::shared_mutex> life(life_);
  std::lock_guard<std::mutex> g(set_mu_);
  if (id < 0 || id >= 16 || !sets_[id].live) return;
  if (sets_[id].stored && ctx_ && jg_set_free) (void)jg_set_free(ctx_, (uint32_t)id);
  sets_[id] = SetRecord{};
}

Engine::SetInfo Engine::set_info(int id) {
  std::shared_lock<std::shared_mutex> life(life_);
  SetInfo out;
  jg_setinfo i{};
  if (ctx_ && jg_set_info && jg_set_info(ctx_, (uint32_t)id, &i) == 0)
    out = SetInfo{i.n, i.nslots, i.maxprobe, i.seed, i.pool_bytes, i.generation};
  return out;
}

// ---- ClaimSet ----
namespace {
std::mutex g_set_tokens_mu;
std::unordered_map<uint32_t, std::weak_ptr<ClaimSetImpl>> g_set_tokens;
uint32_t g_next_set_token = 1;

bool set_member_ok(const std::string& m) {
  if (m.size() > JG_SET_MEMBER_MAX) return false;
  for (unsigned char c : m)
    if (!(c >= 0x20 && c <= 0x7e && c != '"' && c != '\\')) return false;
  return true;
}
uint32_t random_seed() {
  std::random_device rd;
  return (uint32_t)rd();
}
// the members as both paths take them: the host copy, the distinct ones in order, and whether the device takes all
void split_members(const std::vector<std::string>& members, std::shared_ptr<const HostSet>* host, std::vector<std::string>* distinct,
                   bool* host_only) {
  HostSet::Part all;
  *host_only = false;
  for (const std::string& m : members) {
    if (m.find('\0') != std::string::npos) throw std::invalid_argument("capjwt: a claim set member holds a NUL byte");
    if (!all.insert(m).second) continue;
    distinct->push_back(m);
    if (!set_member_ok(m)) *host_only = true;
  }
  *host = HostSet::of(std::move(all));
}
}  // namespace

void ClaimSet::Replace(const std::vector<std::string>& members, std::optional<uint32_t> seed) {
  if (!impl) throw std::invalid_argument("capjwt: an empty ClaimSet handle");
  std::shared_ptr<const HostSet> host;
  std::vector<std::string> distinct;
  bool host_only = false;
  split_members(members, &host, &distinct, &host_only);
  std::lock_guard<std::mutex> g(impl->mu);
  if (impl->closed) throw std::invalid_argument("capjwt: the claim set is closed");
  // a host-only set keeps its id with nothing in it: a scan that captured the id before sees a set, never a hole
  impl->eng->set_store(impl->id, host_only ? std::vector<std::string>() : distinct, seed ? *seed : random_seed());
  impl->host = std::move(host);
  impl->host_only = host_only;
}

size_t ClaimSet::Add(const std::vector<std::string>& members) {
  if (!impl) throw std::invalid_argument("capjwt: an empty ClaimSet handle");
  for (const std::string& m : members)
    if (m.find('\0') != std::string::npos) throw std::invalid_argument("capjwt: a claim set member holds a NUL byte");
  std::lock_guard<std::mutex> g(impl->mu);
  if (impl->closed) throw std::invalid_argument("capjwt: the claim set is closed");
  // only what the set does not hold goes on: the device's pool does not grow from repeats
  HostSet::Part fresh;
  std::vector<std::string> order;
  bool refused = false;
  for (const std::string& m : members) {
    if (impl->host->count(m) || !fresh.insert(m).second) continue;
    order.push_back(m);
    if (!set_member_ok(m)) refused = true;
  }
  if (order.empty()) return 0;
  if (!impl->host_only) {
    // a member the device refuses: host-only from here on, as Replace with the union -- the id kept with nothing in it
    if (refused) impl->eng->set_store(impl->id, std::vector<std::string>(), random_seed());
    else impl->eng->set_add(impl->id, order);
    impl->host_only = refused;
  }
  impl->host = impl->host->with(std::move(fresh));
  return order.size();
}

void ClaimSet::Close() {
  if (!impl) return;
  std::lock_guard<std::mutex> g(impl->mu);
  if (impl->closed) return;
  impl->closed = true;
  impl->eng->set_release(impl->id);
}

size_t ClaimSet::size() const {
  if (!impl) return 0;
  std::lock_guard<std::mutex> g(impl->mu);
  return impl->host ? impl->host->size() : 0;
}

ClaimSet::Info ClaimSet::info() const {
  Info out;
  if (!impl) return out;
  std::lock_guard<std::mutex> g(impl->mu);
  out.n = impl->host ? impl->host->size() : 0;
  out.host_only = impl->host_only;
  if (!impl->closed && !impl->host_only) {
    const Engine::SetInfo i = impl->eng->set_info(impl->id);
    out.nslots = i.nslots;
    out.maxprobe = i.maxprobe;
    out.seed = i.seed;
    out.pool_bytes = i.pool_bytes;
    out.generation = i.generation;
  }
  return out;
}

uint32_t ClaimSet::token() const { return impl ? impl->token : 0; }

ClaimSet ClaimSet::from_token(uint32_t token) {
  ClaimSet s;
  std::lock_guard<std::mutex> g(g_set_tokens_mu);
  auto it = g_set_tokens.find(token);
  if (it != g_set_tokens.end()) s.impl = it->second.lock();
  return s;
}

ClaimSet Validator::NewClaimSet(const std::vector<std::string>& members, std::optional<uint32_t> seed) {
  std::shared_ptr<const HostSet> host;
  std::vector<std::string> distinct;
  bool host_only = false;
  split_members(members, &host, &distinct, &host_only);   // throws before an id is taken
  Engine& eng = ks_->engine();
  ClaimSet s;
  s.impl = std::make_shared<ClaimSetImpl>();
  s.impl->eng = &eng;
  s.impl->id = eng.set_acquire();
  try {
    eng.set_store(s.impl->id, host_only ? std::vector<std::string>() : distinct, seed ? *seed : random_seed());
  } catch (...) {
    eng.set_release(s.impl->id);
    s.impl->id = -1;
    throw;
  }
  s.impl->host = std::move(host);
  s.impl->host_only = host_only;
  std::lock_guard<std::mutex> g(g_set_tokens_mu);
  for (auto it = g_set_tokens.begin(); it != g_set_tokens.end();) it = it->second.expired() ? g_set_tokens.erase(it) : std::next(it);
  s.impl->token = g_next_set_token++;
  g_set_tokens[s.impl->token] = s.impl;
  return s;
}

void Engine::claims_scan(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expect,
                         uint8_t* codes, bool inside_verify) {
  abi_call("jg_claims_scan", jg_claims_scan != nullptr, inside_verify, [&] {
    return jg_claims_scan(ctx_, arena, arena_len, (const jg_cjob*)jobs, njobs, (const jg_expect*)expect, codes);
  });
}

void Engine::claims_extract(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expect,
                            uint8_t* codes, void* vals, bool inside_verify) {
  abi_call("jg_claims_extract", jg_claims_extract != nullptr, inside_verify, [&] {
    return jg_claims_extract(ctx_, arena, arena_len, (const jg_cjob*)jobs, njobs, (const jg_expect*)expect, codes,
                             (jg_claims*)vals);
  });
}

void Engine::claims_select(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expect,
                           const void* select, uint8_t* codes, void* vals, void* sels, bool inside_verify) {
  abi_call("jg_claims_select", jg_claims_select != nullptr, inside_verify, [&] {
    return jg_claims_select(ctx_, arena, arena_len, (const jg_cjob*)jobs, njobs, (const jg_expect*)expect,
                            (const jg_select*)select, codes, (jg_claims*)vals, (jg_selected*)sels);
  });
}

void Engine::claims_each(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expects,
                         uint32_t nexpect, const void* select, uint8_t* codes, void* vals, void* sels,
                         bool inside_verify) {
  abi_call("jg_claims_each", jg_claims_each != nullptr, inside_verify, [&] {
    return jg_claims_each(ctx_, arena, arena_len, (const jg_cjob*)jobs, njobs, (const jg_expect*)expects, nexpect,
                          (const jg_select*)select, codes, (jg_claims*)vals, (jg_selected*)sels);
  });
}

void Engine::claims_paths(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expects,
                          uint32_t nexpect, const void* paths, uint8_t* codes, void* vals, void* sels,
                          bool inside_verify) {
  abi_call("jg_claims_paths", jg_claims_paths != nullptr, inside_verify, [&] {
    return jg_claims_paths(ctx_, arena, arena_len, (const jg_cjob*)jobs, njobs, (const jg_expect*)expects, nexpect,
                           (const jg_paths*)paths, codes, (jg_claims*)vals, (jg_selected*)sels);
  });
}

void Engine::claims_match(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expects,
                          uint32_t nexpect, const void* paths, const void* preds, uint8_t* codes, uint32_t* masks,
                          bool inside_verify) {
  abi_call("jg_claims_match", jg_claims_match != nullptr, inside_verify, [&] {
    return jg_claims_match(ctx_, arena, arena_len, (const jg_cjob*)jobs, njobs, (const jg_expect*)expects, nexpect,
                           (const jg_paths*)paths, (const jg_preds*)preds, codes, masks);
  });
}

void Engine::claims_match_args(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs,
                               const void* expects, uint32_t nexpect, const void* paths, const void* preds,
                               const void* args, uint8_t* codes, uint32_t* masks, bool inside_verify) {
  abi_call("jg_claims_match_args", jg_claims_match_args != nullptr, inside_verify, [&] {
    return jg_claims_match_args(ctx_, arena, arena_len, (const jg_cjob*)jobs, njobs, (const jg_expect*)expects, nexpect,
                                (const jg_paths*)paths, (const jg_preds*)preds, (const jg_args*)args, codes, masks);
  });
}

void Engine::claims_match_hash(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs,
                               const void* expects, uint32_t nexpect, const void* paths, const void* preds,
                               const void* args, const void* hargs, uint8_t* codes, uint32_t* masks,
                               bool inside_verify) {
  abi_call("jg_claims_match_hash", jg_claims_match_hash != nullptr, inside_verify, [&] {
    return jg_claims_match_hash(ctx_, arena, arena_len, (const jg_cjob*)jobs, njobs, (const jg_expect*)expects, nexpect,
                                (const jg_paths*)paths, (const jg_preds*)preds, (const jg_args*)args,
                                (const jg_hargs*)hargs, codes, masks);
  });
}

namespace {

// unicode.IsPrint for the runes an alg header can carry: ASCII graphic + space,
// and every other rune except the C0/C1 controls and the common non-printing
// format / separator runes (Go's tables list more unassigned code points; an
// alg name with those is not a supported alg either way, only its %q differs).
bool go_is_print(uint32_t r) {
  if (r < 0x80) return r >= 0x20 && r < 0x7f;
  if (r < 0xa0 || r == 0xad) return false;
  if (r == 0xa0 || r == 0x1680 || (r >= 0x2000 && r <= 0x200f) || (r >= 0x2028 && r <= 0x202f) ||
      (r >= 0x205f && r <= 0x2064) || r == 0x3000 || r == 0xfeff || (r >= 0xfff9 && r <= 0xfffb) ||
      r == 0xfffe || r == 0xffff || (r >= 0xd800 && r <= 0xdfff) || r > 0x10ffff)
    return false;
  return true;
}

// fmt %q of a string (strconv.Quote)
std::string go_quote(std::string_view s) {
  static const char* hex = "0123456789abcdef";
  std::string o = "\"";
  size_t i = 0;
  while (i < s.size()) {
    size_t w = 1;
    const uint32_t r = json::decode_rune((const unsigned char*)s.data() + i, s.size() - i, &w);
    if (r == 0xfffd && w == 1) {                       // invalid byte
      const unsigned char b = (unsigned char)s[i];
      o += "\\x";
      o.push_back(hex[b >> 4]);
      o.push_back(hex[b & 15]);
    } else if (r == '"' || r == '\\') {
      o.push_back('\\');
      o.push_back((char)r);
    } else if (go_is_print(r)) {
      o.append(s.substr(i, w));
    } else if (r == '\a') { o += "\\a"; } else if (r == '\b') { o += "\\b"; } else if (r == '\f') { o += "\\f"; }
    else if (r == '\n') { o += "\\n"; } else if (r == '\r') { o += "\\r"; } else if (r == '\t') { o += "\\t"; }
    else if (r == '\v') { o += "\\v"; }
    else if (r < ' ' || r == 0x7f) {
      o += "\\x";
      o.push_back(hex[r >> 4]);
      o.push_back(hex[r & 15]);
    } else {
      const int nd = r < 0x10000 ? 4 : 8;
      o += nd == 4 ? "\\u" : "\\U";
      for (int k = nd - 1; k >= 0; --k) o.push_back(hex[(r >> (4 * k)) & 15]);
    }
    i += w;
  }
  o.push_back('"');
  return o;
}

// oidc.UnmarshalClaims(rawToken, &map[string]interface{})   (oidc/token.go:170-184)
bool unmarshal_claims(std::string_view raw, json::Value* claims, std::string* err) {
  size_t parts = 1;
  for (char c : raw) parts += c == '.';
  if (parts != 3) {
    *err = "UnmarshalClaims: malformed jwt, expected 3 parts got " + std::to_string(parts) + ": invalid parameter";
    return false;
  }
  const size_t d1 = raw.find('.'), d2 = raw.find('.', d1 + 1);
  std::string payload, e;
  if (!b64rawurl_decode(raw.substr(d1 + 1, d2 - d1 - 1), &payload, &e)) {
    *err = "UnmarshalClaims: malformed jwt claims: " + e;
    return false;
  }
  if (!claims_map(payload, claims, &e)) {
    *err = "UnmarshalClaims: unable to marshal jwt JSON: " + e;
    return false;
  }
  return true;
}

struct HashPlan {
  int fam = 0;                   // jg_hash_fam, 0 = no hash (decided already)
  std::string want;              // the claim's value
};

// verifyHashClaim up to the hash: fills r (decided) or p (hash needed)
void hash_claim_plan(const std::string& claim, std::string_view t, HashClaimResult* r, HashPlan* p) {
  const std::string op = "verifyHashClaim";
  json::Value claims;
  std::string e;
  if (t.empty()) {
    r->err = op + ": IDToken.Claims: id_token is empty: invalid parameter";
    return;
  }
  if (!unmarshal_claims(t, &claims, &e)) {
    r->err = op + ": " + e;
    return;
  }
  const json::Value* v = claims.kind == json::Value::Object ? claims.get(claim) : nullptr;
  if (!v || v->kind != json::Value::String) return;        // (false, nil)
  JWS jws;
  if (!parse_signed(t, &jws, &e)) {
    r->err = op + ": malformed jwt (" + e + "): token malformed";
    return;
  }
  if (jws.sigs.empty()) {
    r->err = op + ": id_token not signed: token is not signed";
    return;
  }
  if (jws.sigs.size() > 1) {
    r->err = op + ": multiple signatures on id_token not supported";
    return;
  }
  const int alg = alg_id(jws.sigs[0].alg);
  if (!alg) {
    r->err = op + ": id_token signed with algorithm " + go_quote(jws.sigs[0].alg) + ": unsupported signing algorithm";
    return;
  }
  switch (alg) {
    case JG_RS256: case JG_ES256: case JG_PS256: p->fam = JG_SHA256; break;
    case JG_RS384: case JG_ES384: case JG_PS384: p->fam = JG_SHA384; break;
    case JG_RS512: case JG_ES512: case JG_PS512: p->fam = JG_SHA512; break;
    default: return;                                        // EdDSA: (false, nil)
  }
  p->want = v->str;
}

std::vector<HashClaimResult> verify_hash_claim_batch(Engine& eng, const std::string& claim,
                                                     const std::vector<std::string_view>& id_tokens,
                                                     const std::vector<std::string_view>& values) {
  if (id_tokens.size() != values.size()) throw std::invalid_argument("id_tokens and values differ in length");
  const size_t n = id_tokens.size();
  std::vector<HashClaimResult> out(n);
  std::vector<HashPlan> plan(n);
  parallel_for(n, host_threads(), [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) hash_claim_plan(claim, id_tokens[i], &out[i], &plan[i]);
  });
  // one GPU batch over the values that need hashing
  std::vector<size_t> idx;
  size_t bytes = 0;
  for (size_t i = 0; i < n; ++i)
    if (plan[i].fam) {
      idx.push_back(i);
      bytes += values[i].size();
    }
  if (!idx.empty()) {
    std::string arena;
    arena.reserve(bytes);
    std::vector<jg_hjob> jobs(idx.size());
    for (size_t k = 0; k < idx.size(); ++k) {
      jobs[k] = jg_hjob{};
      jobs[k].off = arena.size();
      jobs[k].len = (uint32_t)values[idx[k]].size();
      jobs[k].fam = (uint8_t)plan[idx[k]].fam;
      arena.append(values[idx[k]]);
    }
    std::vector<uint8_t> dig(64 * idx.size());
    try {
      eng.hash((const uint8_t*)arena.data(), arena.size(), jobs.data(), jobs.size(), dig.data());
    } catch (const DeviceError& e) {
      // degraded path, as the key sets': the pairs that needed the device get
      // its error, the batch returns, and the context is recreated for the next
      for (size_t i : idx) out[i].err = std::string("capjwt: hash unavailable: ") + e.what();
      idx.clear();
      (void)eng.recover(eng.errors());
    }
    parallel_for(idx.size(), host_threads(), [&](size_t lo, size_t hi) {
      for (size_t k = lo; k < hi; ++k) {
        const size_t i = idx[k];
        const size_t half = (plan[i].fam == JG_SHA256 ? 32 : plan[i].fam == JG_SHA384 ? 48 : 64) / 2;
        const std::string actual = b64url_encode(std::string_view((const char*)dig.data() + 64 * k, half));
        if (actual != plan[i].want) {
          out[i].err = claim == "at_hash" ? "verifyHashClaim: access_token hash does not match value in id_token"
                                          : "verifyHashClaim: authorization code hash does not match value in id_token";
        } else {
          out[i].verified = true;
        }
      }
    });
  }
  for (auto& r : out)
    if (!r.err.empty()) r.err = "VerifyAccessToken: " + r.err;     // both public methods use this op
  return out;
}

}  // namespace

std::vector<HashClaimResult> VerifyAccessTokenBatch(Engine& eng, const std::vector<std::string_view>& id_tokens,
                                                    const std::vector<std::string_view>& access_tokens) {
  return verify_hash_claim_batch(eng, "at_hash", id_tokens, access_tokens);
}

std::vector<HashClaimResult> VerifyAuthorizationCodeBatch(Engine& eng, const std::vector<std::string_view>& id_tokens,
                                                          const std::vector<std::string_view>& codes) {
  return verify_hash_claim_batch(eng, "c_hash", id_tokens, codes);
}

}  // namespace capjwt
