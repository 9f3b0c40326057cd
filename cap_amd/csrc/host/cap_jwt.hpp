// cap_jwt.hpp -- C++ mirror of cap's jwt package API (jwt/keyset.go, jwt/jwt.go,
// jwt/algs.go) on top of the GPU verifier's C ABI (include/jg.h).
//
// Go is absent from this image, so this layer stands where the Go host code of
// BASELINE.json's north star would: it keeps base64url/JSON header parsing,
// kid -> key lookup and claims validation on the host and hands every
// signature check to libcapjwt.so in one batch.  Names, argument meaning and
// error strings follow the reference:
//
//   Go (reference)                                   here
//   KeySet.VerifySignature    jwt/keyset.go:27-32     KeySet::VerifySignature / VerifySignatureBatch
//   NewStaticKeySet           jwt/keyset.go:142-150   NewStaticKeySet
//   NewJSONWebKeySet          jwt/keyset.go:109-123   NewJSONWebKeySet (HTTP GET via a Fetcher)
//   NewOIDCDiscoveryKeySet    jwt/keyset.go:49-104    NewOIDCDiscoveryKeySet
//   ParsePublicKeyPEM         jwt/keyset.go:178-200   ParsePublicKeyPEM
//   NewValidator / Validate   jwt/jwt.go:25-202       NewValidator / Validator::Validate
//   (north star) ValidateBatch                        Validator::ValidateBatch
//   (verdict only) CheckBatch                         Validator::CheckBatch (claims scanned on the GPU)
//   jwt.Claims after Validate jwt/jwt.go:107-116      Validator::RegisteredBatch (verdict + registered claims
//                                                     from the GPU scan, no claims map)
//   SupportedSigningAlgorithm jwt/algs.go:38-46       SupportedSigningAlgorithm
//
// There is no CPU verification path: a KeySet whose GPU context cannot be
// created fails at construction.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_set>
#include <vector>

#include "jose.hpp"
#include "json.hpp"

struct jg_ctx;

namespace capjwt {

// ---------------------------------------------------------------- algs (jwt/algs.go)
extern const char* const kSupportedAlgorithms[10];
// "" if every alg is supported, else `unsupported signing algorithm "X"`
std::string SupportedSigningAlgorithm(const std::vector<std::string>& algs);

// ---------------------------------------------------------------- results
// (claims, error): ok == true <=> Go's err == nil.  claims is the
// map[string]interface{} (Object) or nil (Null, for a `null` payload).
struct Result {
  bool ok = false;
  json::Value claims;
  std::string err;
};

// ---------------------------------------------------------------- batch arrays
// Runs fn(begin, end) over [0, n) on `threads` host threads (contiguous ranges;
// small n stays on the caller's thread).
void batch_parallel(size_t n, int threads, const std::function<void(size_t, size_t)>& fn);
int host_threads();

// Storage of the batch arrays (BatchArray, the key sets' per-token records):
// blocks of 1 MiB and more come from the hostmem pool (hostmem.hpp) and go
// back to it when freed, instead of going back to the OS.  A 1M-token batch
// frees ~200 MB of records twice per ValidateBatch call; returned to the OS
// each time, the unmap cost ~30 ms per array and the next call paid the page
// faults again (bench e2e phases "free-toks", "blob release").  A pooled
// block is reused for a request of at least half its size; *cap receives the
// block's true capacity, which batch_block_free takes back.
void* batch_block_alloc(size_t bytes, size_t* cap);
void batch_block_free(void* p, size_t cap);

// Host memory the batches keep for reuse (hostmem pools): at most `bytes`
// (default 4 GiB, or CAPJWT_HOST_CACHE_GB); TrimHostMemory hands all of it
// back to the OS now.  HostMemoryRetained: bytes held right now.
void SetHostMemoryRetention(size_t bytes);
void TrimHostMemory();
size_t HostMemoryRetained();

// The per-token records of a batch, constructed and destroyed by all host
// threads: a 1M-token batch's results are ~150 MB of records plus their claims
// maps, and a serial std::vector construction or free of that costs more than
// the batch's parse.  Move-only; indexable and iterable like a vector.  The
// array also owns the arenas its records' claims trees live in (adopt): they
// are released after the records.
template <class T>
class BatchArray {
 public:
  BatchArray() = default;
  explicit BatchArray(size_t n, int threads = host_threads()) : threads_(threads) {
    p_ = static_cast<T*>(batch_block_alloc(sizeof(T) * (n ? n : 1), &cap_));
    batch_parallel(n, threads_, [this](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) new (p_ + i) T();
    });
    n_ = n;
  }
  BatchArray(BatchArray&& o) noexcept
      : p_(o.p_), n_(o.n_), cap_(o.cap_), threads_(o.threads_), arenas_(std::move(o.arenas_)) {
    o.p_ = nullptr; o.n_ = 0;
  }
  BatchArray& operator=(BatchArray&& o) noexcept {
    if (this != &o) {
      release();
      p_ = o.p_; n_ = o.n_; cap_ = o.cap_; threads_ = o.threads_; arenas_ = std::move(o.arenas_);
      o.p_ = nullptr; o.n_ = 0;
    }
    return *this;
  }
  BatchArray(const BatchArray&) = delete;
  BatchArray& operator=(const BatchArray&) = delete;
  ~BatchArray() { release(); }
  void release() {
    if (p_) {
      batch_parallel(n_, threads_, [this](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) p_[i].~T();
      });
      batch_block_free(p_, cap_);
    }
    p_ = nullptr;
    n_ = 0;
    arenas_.clear();
  }
  // keep `a` alive as long as the records (thread-safe)
  void adopt(std::unique_ptr<json::Arena> a) {
    std::lock_guard<std::mutex> g(amu_);
    arenas_.push_back(std::move(a));
  }
  T& operator[](size_t i) { return p_[i]; }
  const T& operator[](size_t i) const { return p_[i]; }
  size_t size() const { return n_; }
  T* begin() { return p_; }
  T* end() { return p_ + n_; }
  const T* begin() const { return p_; }
  const T* end() const { return p_ + n_; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0, cap_ = 0;
  int threads_ = 1;
  std::vector<std::unique_ptr<json::Arena>> arenas_;
  std::mutex amu_;
};
using Results = BatchArray<Result>;

// ---------------------------------------------------------------- HTTP
// The JWKS / discovery GET.  The reference uses net/http with a TLS client
// built from the CA PEM (createCAContext, jwt/keyset.go:204-227); here the
// caller supplies the transport.  Throw std::runtime_error for a transport
// error (Go: client.Do error).
struct FetchResponse {
  int status = 200;
  std::string status_text = "200 OK";   // resp.Status
  std::string body;
  std::string content_type = "application/json";
  int64_t max_age_s = -1;               // Cache-Control max-age; -1 = none (go-oidc: expire at once)
};
using Fetcher = std::function<FetchResponse(const std::string& url, const std::string& ca_pem)>;

// ---------------------------------------------------------------- GPU engine
// A failed device call: jg_* returned -2 (a HIP error, a lost device).  The key
// sets turn it into per-token errors and recover the context (Engine::recover).
// A -1 (a job outside the key table or the arena: the host layer packed it
// wrong) is a std::logic_error and propagates -- it is a bug, not a device fault.
struct DeviceError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// One jg_ctx (HIP devices + staged key table).  Thread-safe: concurrent verify
// calls are separate submissions that pipeline on the devices (jg_submit).
class Engine {
 public:
  explicit Engine(const std::vector<int>& devices);
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;
  void load(const std::vector<PublicKey>& keys);      // jg_keys_load (returns once the keys verify)
  void wait_tables();                                 // jg_keys_wait_tables: wide comb tables in place
  // verify (arena entry, key, alg) jobs; verdicts[i] = 1 accept, 0 reject.
  // `submitted` runs once the jobs are queued (before the wait): a key set
  // releases its key-list lock there, so refreshes never wait for the device.
  void verify(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, uint8_t* verdicts,
              const std::function<void()>& submitted = {});
  // SHA-2 of (arena span, family) jobs: digests njobs x 64 bytes (jg_hash_batch)
  void hash(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, uint8_t* digests);
  // registered-claims scan of (arena span) jobs against one resolved Expected
  // (jg_cjob / jg_expect): codes[i] = a jg_claim_code (jg_claims_scan).
  // inside_verify: called from verify()'s `submitted` callback, on its thread
  // (that call already holds the context's lifetime lock).
  void claims_scan(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expect,
                   uint8_t* codes, bool inside_verify = false);
  // ... and vals[i] = the jg_claims record of job i (jg_claims_extract)
  void claims_extract(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expect,
                      uint8_t* codes, void* vals, bool inside_verify = false);
  // ... and sels[i] = the jg_selected record of the members `select` (a
  // jg_select) names (jg_claims_select)
  void claims_select(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expect,
                     const void* select, uint8_t* codes, void* vals, void* sels, bool inside_verify = false);
  // The three scans with a profile per job (jg_claims_each): `expects` is
  // nexpect jg_expect and a job's flags names its own; sels (with select and
  // vals) asks for claims_select's outputs, else vals for claims_extract's
  void claims_each(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expects,
                   uint32_t nexpect, const void* select, uint8_t* codes, void* vals, void* sels,
                   bool inside_verify = false);
  // jg_claims_each's selecting form for members named by path (jg_claims_paths):
  // `paths` is a jg_paths
  void claims_paths(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expects,
                    uint32_t nexpect, const void* paths, uint8_t* codes, void* vals, void* sels,
                    bool inside_verify = false);
  // jg_claims_each's codes and masks[i] = the predicates of `preds` (a jg_preds
  // over `paths`, a jg_paths) that hold on job i's claims (jg_claims_match)
  void claims_match(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expects,
                    uint32_t nexpect, const void* paths, const void* preds, uint8_t* codes, uint32_t* masks,
                    bool inside_verify = false);
  // ... with the jobs' own operands (`args`, a jg_args) for the ops that take one (jg_claims_match_args)
  void claims_match_args(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expects,
                         uint32_t nexpect, const void* paths, const void* preds, const void* args, uint8_t* codes,
                         uint32_t* masks, bool inside_verify = false);
  // ... and with hash columns (`hargs`, a jg_hargs) whose operands the device makes (jg_claims_match_hash)
  void claims_match_hash(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expects,
                         uint32_t nexpect, const void* paths, const void* preds, const void* args, const void* hargs,
                         uint8_t* codes, uint32_t* masks, bool inside_verify = false);
  // ... and with resident sets (`sets`, a jg_setargs) for InSet / AnyElementIn (jg_claims_match_set)
  void claims_match_set(const uint8_t* arena, size_t arena_len, const void* jobs, size_t njobs, const void* expects,
                        uint32_t nexpect, const void* paths, const void* preds, const void* args, const void* hargs,
                        const void* sets, uint8_t* codes, uint32_t* masks, bool inside_verify = false);
  // Resident sets (jg_set_load / jg_set_free / jg_set_info), ids 0..15 of the
  // context.  set_acquire() hands out a free id or throws for the 17th live set;
  // set_store() loads `members` (device-legal, distinct) under `seed` and keeps
  // them, so that recover() can load the set again into a new context; a failure
  // throws and leaves what the id held before.  set_release() frees the id.
  struct SetInfo {
    uint32_t n = 0, nslots = 0, maxprobe = 0, seed = 0;
    uint64_t pool_bytes = 0, generation = 0;
  };
  int set_acquire();
  void set_store(int id, const std::vector<std::string>& members, uint32_t seed);
  // set_add() adds `members` (device-legal, distinct, none of them in the set) to
  // the stored set on the device (jg_set_add) and to what recover() loads again;
  // with a library that lacks jg_set_add the union is loaded whole (jg_set_load).
  // A failure throws runtime_error and leaves what the id held before.
  void set_add(int id, const std::vector<std::string>& members);
  void set_release(int id);
  SetInfo set_info(int id);
  // Pinned host memory for one call's arena (jg_host_alloc), from a small pool
  // of blocks the engine keeps; back to the pool when the Pinned dies.
  class Pinned {
   public:
    Pinned(Engine* e, uint8_t* p, size_t cap) : e_(e), p_(p), cap_(cap) {}
    Pinned(Pinned&& o) noexcept : e_(o.e_), p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; }
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned();
    uint8_t* get() const { return p_; }
   private:
    Engine* e_;
    uint8_t* p_;
    size_t cap_;
  };
  Pinned pinned(size_t bytes);
  // Recreate the device context after a DeviceError: its streams and
  // per-device state are torn down and rebuilt and the current key list is
  // re-staged (no process restart, no key refetch).  `seen` = errors() when
  // the caller's call failed: a recovery since then is not repeated.  True
  // when the engine verifies again; false leaves it marked lost (status()).
  bool recover(uint64_t seen);
  uint64_t errors() const { return errors_.load(); }  // DeviceErrors so far
  int recoveries() const { return recoveries_.load(); }
  std::string status();                               // "" healthy, else why the device is lost
  int debug_fail_verify(int n);                       // jg_debug_fail_verify (test hook)
  int threads() const { return threads_; }
 private:
  void fail_device(const std::string& what);          // count the error; throws DeviceError
  // One call of the ABI entry `name` on ctx_ (call(): its return code), under
  // the lifetime lock unless inside_verify.  -1 is a logic_error, a lost
  // context, an entry the library does not provide (!present) or any other
  // code a DeviceError.
  template <class F>
  void abi_call(const char* name, bool present, bool inside_verify, F&& call);
  std::vector<int> devices_;
  jg_ctx* ctx_ = nullptr;
  std::shared_mutex life_;        // shared: calls on ctx_; unique: recover (ctx_ replaced)
  std::mutex load_mu_;            // serialises loads; guards keys_
  std::vector<PublicKey> keys_;   // the list the context holds (re-staged by recover)
  struct SetRecord {              // a live id: what it holds (loaded again by recover), under set_mu_
    bool live = false, stored = false;
    std::string bytes;
    std::vector<std::pair<uint32_t, uint32_t>> spans;
    uint32_t seed = 0;
  };
  std::mutex set_mu_;
  SetRecord sets_[16];
  int set_load_locked(int id);    // jg_set_load of sets_[id] into ctx_: its return code
  bool has_keys_ = false;
  std::atomic<uint64_t> errors_{0};
  uint64_t recovered_at_ = 0;     // errors_ when the last recovery ran (under life_)
  std::atomic<int> recoveries_{0};
  std::string lost_;              // why ctx_ is null (under life_)
  std::chrono::steady_clock::time_point last_try_{};
  std::mutex pin_mu_;
  std::vector<std::pair<uint8_t*, size_t>> pin_free_;
  int threads_ = 1;
};

// ---------------------------------------------------------------- KeySet
struct TokenInfo {          // what validateSigningAlgorithm needs from ParseSigned
  bool parsed = false;
  std::string parse_err;
  size_t nsigs = 0;
  size_t sig0_len = 0;
  std::string alg;
};
// The same, as views into a batch's parse records (valid during a PostFn call)
struct TokenView {
  bool parsed = false;
  std::string_view parse_err;
  size_t nsigs = 0;
  size_t sig0_len = 0;
  std::string_view alg;
};
// Per-token continuation of a batch verify: called on the host threads, once
// per token (i = its index in the batch), right after that token's (claims,
// error) is final -- the Validator's claim checks run there while the claims
// map is still in cache.
using PostFn = std::function<void(size_t i, Result& r, const TokenView& t)>;

// Request coalescing of single-token calls (KeySet::VerifySignature,
// Validator::Validate, RemoteKeySet::VerifySignature): a Go service calls
// these once per request from many goroutines.  Each call queues its token;
// while fewer than `max_inflight` batches are on the device, a caller takes
// everything queued (up to `max_batch` tokens, after waiting at most
// `window_us` for more to arrive) and runs it as ONE batch, then wakes the
// callers it carried.  Under load the batches grow by themselves (everything
// that arrived while the device was busy goes in the next); an idle device
// takes a lone token at once.  No lock is held across a device call.
struct CoalesceConfig {
  int max_inflight = 4;
  size_t max_batch = 65536;
  int64_t window_us = 0;
};
struct Verified;                  // a batch after parse and device verification (cap_jwt.cpp)
class Coalescer {
 public:
  struct Req {
    std::string_view tok;
    std::shared_ptr<const Verified> batch;   // the verified batch that carried this token ...
    size_t idx = 0;                          // ... and its index there
    std::exception_ptr ex;        // the batch threw (a host-side bug): re-thrown to every caller in it
    std::shared_ptr<std::vector<Req*>> peers;   // the batch's callers to wake (a binary tree) ...
    size_t wpos = 0;                            // ... and this one's position there
    Req* next = nullptr;          // the submission stack's link
    enum { WAITING = 0, DONE = 1 };
    std::atomic<int> state{WAITING};   // futex word: DONE once a dispatcher has carried it
  };
  // parse + verify a batch of tokens (KeySet::verify_raw)
  using Exec = std::function<std::shared_ptr<const Verified>(const std::vector<std::string_view>&)>;
  explicit Coalescer(Exec exec) : exec_(std::move(exec)) {}
  ~Coalescer();
  void run(Req* r);               // blocks until r->batch is set (exceptions of the batch re-thrown)
  void configure(const CoalesceConfig& c);
  CoalesceConfig config();
  struct Stats { uint64_t calls = 0, batches = 0, max_batch_seen = 0; };
  Stats stats();
 private:
  static void release(const std::vector<Req*>& wake, size_t i);
  void dispatch_loop();
  void serve_stack(std::vector<Req*>& all, std::vector<Req*>& batch);   // one exchange of the stack, carried
  void carry(std::vector<Req*>& batch);
  void kick();                    // wake one idle dispatcher
  void start_locked();            // spawn the dispatchers (threads_mu_ held)
  void stop_locked();             // stop and join them (threads_mu_ held)
  Exec exec_;
  std::atomic<Req*> head_{nullptr};        // submissions not yet taken (LIFO, lock-free)
  std::atomic<uint32_t> seq_{0};           // futex word of idle dispatchers (kick)
  std::atomic<int> active_{0};             // batches being carried (callers leading + dispatchers)
  std::atomic<int> max_inflight_{4};
  std::atomic<bool> stop_{false};
  std::atomic<bool> started_{false};
  std::mutex threads_mu_;
  std::vector<std::thread> threads_;
  CoalesceConfig cfg_;                      // threads_mu_
  std::atomic<size_t> max_batch_{65536};
  std::atomic<int64_t> window_us_{0};
  std::atomic<uint64_t> calls_{0}, batches_{0}, max_seen_{0};
};

class KeySet {
 public:
  KeySet();
  virtual ~KeySet() = default;
  // jwt/keyset.go:27-32 (one token; concurrent calls are coalesced into
  // batches, and each caller builds its own claims map on its own thread)
  Result VerifySignature(std::string_view token);
  Results VerifySignatureBatch(const std::vector<std::string_view>& tokens);
  // batch verify; `post` (may be null) continues each token's result with what
  // the parse learned (Validator::ValidateBatch)
  Results verify_batch(const std::vector<std::string_view>& tokens, const PostFn* post);
  // one token through the coalescer, with its parse info (Validator::Validate)
  Result verify_one(std::string_view token, TokenInfo* info);
  // the two halves of a batch: parse + device verification, then token i's
  // (claims, error) -- the key set's own error strings and JSON rules
  // overlap (may be null): run while the batch's device call is in flight
  // (after parse, before the verdicts) -- verify_batch parses the claims then
  using Overlap = std::function<void(const Verified&)>;
  virtual std::shared_ptr<Verified> verify_raw(const std::vector<std::string_view>& tokens,
                                               const Overlap* overlap = nullptr) = 0;
  virtual void finish(const Verified& V, size_t i, Result& r) = 0;
  // finish() for a parsed token whose claims map was already read into r
  // (json_ok; else r.err holds the JSON error) while the device verified
  virtual void finish_pre(const Verified& V, size_t i, Result& r, bool json_ok) = 0;
  virtual const char* trace_name() const = 0;
  // block until background comb-table widening of the last key load is done
  // (keys verify before that, on narrower tables; a measurement hook)
  virtual void WaitTables() {}
  void SetCoalescing(const CoalesceConfig& c) { co_.configure(c); }
  Coalescer::Stats CoalescingStats() { return co_.stats(); }
  // the device context behind the key set: "" healthy, else why it is lost;
  // how many times it was recovered after a device error
  virtual std::string DeviceStatus() = 0;
  virtual int DeviceRecoveries() = 0;
  virtual int DebugFailVerify(int n) = 0;            // jg_debug_fail_verify on its context (tests)
  virtual Engine& engine() = 0;                      // the device context (Validator::CheckBatch's claims scan)
 private:
  Coalescer co_;
};

std::unique_ptr<KeySet> NewStaticKeySet(const std::vector<PublicKey>& keys, std::string* err,
                                        const std::vector<int>& devices = {});
std::unique_ptr<KeySet> NewJSONWebKeySet(const std::string& jwks_url, const std::string& jwks_ca_pem, Fetcher fetch,
                                         std::string* err, const std::vector<int>& devices = {});
std::unique_ptr<KeySet> NewOIDCDiscoveryKeySet(const std::string& issuer, const std::string& issuer_ca_pem,
                                               Fetcher fetch, std::string* err, const std::vector<int>& devices = {});

// ---------------------------------------------------------------- go-oidc KeySet adapter
// go-oidc v2.2.1's `oidc.KeySet` (VerifySignature(ctx, jwt) ([]byte, error)) as
// returned by oidc.NewRemoteKeySet: the interface cap's jsonWebKeySet wraps
// (jwt/keyset.go:101,120,127) and go-oidc's IDTokenVerifier calls -- the path
// behind cap's oidc.Provider.VerifyIDToken (oidc/provider.go:418-441).  Same
// kid filtering, refresh-on-miss and error strings as the JWKS key set above
// ("oidc: malformed jwt: ...", "failed to verify id token signature",
// "fetching keys ..."), returning the verified payload bytes.
struct PayloadResult {
  bool ok = false;
  std::string payload;
  std::string err;
};
class RemoteKeySet {
 public:
  RemoteKeySet(const std::string& jwks_url, Fetcher fetch, const std::vector<int>& devices);
  ~RemoteKeySet();
  PayloadResult VerifySignature(std::string_view jwt);            // coalesced, as KeySet's
  std::vector<PayloadResult> VerifySignatureBatch(const std::vector<std::string_view>& jwts);
  void SetCoalescing(const CoalesceConfig& c);
 private:
  class Impl;
  std::unique_ptr<Impl> impl_;
};
std::unique_ptr<RemoteKeySet> NewRemoteKeySet(const std::string& jwks_url, Fetcher fetch,
                                              const std::vector<int>& devices = {});

// ---------------------------------------------------------------- Validator
constexpr int64_t kSecond = 1000000000LL;
constexpr int64_t DefaultLeewaySeconds = 150;          // jwt/jwt.go:16

struct Expected {                                      // jwt/jwt.go:38-83
  std::string Issuer, Subject, ID;
  std::vector<std::string> Audiences;
  std::vector<std::string> SigningAlgorithms;
  int64_t NotBeforeLeeway = 0;                         // time.Duration (ns)
  int64_t ExpirationLeeway = 0;
  int64_t ClockSkewLeeway = 0;
  bool has_now = false;                                // Now == nil -> time.Now()
  int64_t now_unix_ns = 0;
};

// Validate's (ok, error string) for one token, without the claims map
struct CheckResult {
  bool ok = false;
  std::string err;
};
// Where a CheckBatch call's claim verdicts came from: tokens whose registered
// claims the device decided / tokens that took the host path (claims map +
// validate_claims).  Tokens that fail before the claims (parse, signature) are
// in neither.
struct CheckStats {
  size_t scanned = 0, host = 0;
};

// go-jose's jwt.Claims after json.Unmarshal (jwt/jwt.go:107-116): what Validate
// itself decodes from the claims map to run its checks
struct RegisteredClaims {
  std::string Issuer, Subject, ID;
  std::vector<std::string> Audience;
  std::optional<int64_t> Expiry, NotBefore, IssuedAt;   // nil for absent or null
};
// Validate's (ok, error string) and, when ok, the registered claims
struct RegisteredResult {
  bool ok = false;
  std::string err;
  RegisteredClaims claims;
};
// RegisteredBatch as columns (RegisteredBlob), written straight into memory the
// caller supplies; no per-token object is built for a token the device decides.
// Rows of a rejected token are empty (zero, and equal offsets).
struct RegisteredColumns {
  // one entry per token
  uint8_t* ok = nullptr;          // 1 = Validate returns no error
  uint8_t* present = nullptr;     // bit 5 exp, 6 nbf, 7 iat: the date is there (not absent, not null)
  int64_t *exp = nullptr, *nbf = nullptr, *iat = nullptr;
  // n + 1 offsets each: token i's string is data[off[i], off[i + 1]); token i's
  // audiences are elements [aud_tok[i], aud_tok[i + 1])
  uint32_t *iss_off = nullptr, *sub_off = nullptr, *jti_off = nullptr, *aud_tok = nullptr;
  // The columns whose size the call finds out: the bytes of iss / sub / jti,
  // of the audience elements back to back, and the elements' offsets (uint32,
  // one more than there are elements).  alloc(which, bytes) is called once for
  // each, from the calling thread, and returns where to write them.
  enum Var { ISS = 0, SUB = 1, JTI = 2, AUD = 3, AUD_OFF = 4 };
  std::function<void*(Var which, size_t bytes)> alloc;
};

// RegisteredResult and the claims the caller named: values[k] is what
// ValidateBatch's claims map holds under names[k] (nullopt: the map has no such
// key; a JSON null is a Value of kind Null).  A rejected token carries none.
struct SelectResult {
  bool ok = false;
  std::string err;
  RegisteredClaims claims;
  std::vector<std::optional<json::Value>> values;     // one per name
};
// A claim inside objects, by the keys that lead to it: {"realm_access", "roles"}
// is claims["realm_access"]["roles"].  Components are literal keys; nothing in
// them is parsed as a separator.
using ClaimPath = std::vector<std::string>;
// The paths of one Select call.  A type of its own, so that a braced list of
// names ({"scope", "roles"}) still names the overload that takes names alone.
struct ClaimPaths {
  std::vector<ClaimPath> paths;
};
// A set of strings a claim can be held against (InSet, AnyElementIn): a deny-list
// of revoked ids, the tenants a gateway serves.  Made by Validator::NewClaimSet
// from the key set that owns the device context; a shared handle that owns one
// of the context's 16 set ids and frees it when the last copy dies (or at
// Close()).  It must not outlive that key set.  The members are any strings
// without a NUL (std::invalid_argument otherwise); a host copy answers the host
// path.  A set all of whose members the device takes -- at most 255 bytes, each
// printable ASCII without quote and backslash -- is resident on the device;
// any other set is host-only (Info().host_only) and every token of a call that
// names it is answered from the host path, so no result depends on it.
struct ClaimSetImpl;
class ClaimSet {
 public:
  struct Info {
    size_t n = 0;                   // distinct members
    bool host_only = false;
    uint32_t nslots = 0, maxprobe = 0, seed = 0;   // of the resident table (0 for a host-only set)
    uint64_t pool_bytes = 0, generation = 0;
  };
  ClaimSet() = default;
  explicit operator bool() const { return (bool)impl; }
  size_t size() const;
  Info info() const;
  // The whole set anew, under the same id.  Any failure (a NUL: invalid_argument;
  // a device allocation or load failure: runtime_error) leaves the old members in
  // force on both paths.  seed: random per load unless given (tests).
  void Replace(const std::vector<std::string>& members, std::optional<uint32_t> seed = std::nullopt);
  // Adds members; returns how many were new.  Only those the set does not hold yet
  // go to the device (jg_set_add: a kernel inserts them into a copy of the resident
  // table, published whole, so a scan in flight keeps the set it captured), and the
  // host copy grows by an overlay, not by a copy: a call costs what it adds, not
  // what the set holds.  A NUL in a member throws invalid_argument before anything
  // changes; any failure (runtime_error) leaves the old members in force on both
  // paths.  A member the device refuses turns the set host-only, as Replace with
  // the union would; Add on a host-only set touches the host copy alone.  Throws
  // after Close().  MatchPlans made before see the set as it was.
  size_t Add(const std::vector<std::string>& members);
  void Close();                     // frees the id now; a later call that names the set throws
  uint32_t token() const;           // a process-wide number of this handle, for bindings: from_token() finds it again
  static ClaimSet from_token(uint32_t token);
  std::shared_ptr<ClaimSetImpl> impl;
};

// A yes/no question about one claim (MatchBatch).  With v the value the claims
// map holds at `path`:
//   Equals      v is a string equal to `value` ("" allowed)
//   HasWord     v is a string and one of strings.Split(v, " ") equals `value`
//               (the RFC 6749 scope form)
//   HasElement  v is an array and one of its direct elements is a string equal
//               to `value`
//   Present     the path reaches a value (null counts); `value` is unused
// ... and, for the MatchBatchArgs entries only, with the token's own operands:
//   EqualsArg   v is a string equal to the token's entry in string column `column`
//   AtLeast     v is a number f with f >= float64(bound); AtMost: f <= float64(bound)
//   AtLeastArg  AtLeast with the token's entry in number column `column` as the
//               bound; AtMostArg likewise
// ... and, for the same entries, the two halves of an OIDC hash-claim check
// (oidc/id_token.go verifyHashClaim; jg_claims_match_hash):
//   HashOfArg   v is a string equal to base64.RawURLEncoding(SHA-2(x)[:size/2]) of
//               the token's entry x in hash column `column`, with the SHA-2 of the
//               token's own alg (RS/ES/PS256 -> SHA-256, 384 -> SHA-384, 512 ->
//               SHA-512); never holds under EdDSA or for an absent entry
//   IsString    v is a string ("" counts; null, numbers, arrays, objects do not)
// Go's (verified, err) of IDToken.VerifyAccessToken is (IsString & HashOfArg,
// err != nil exactly when IsString holds, HashOfArg does not and the alg is not
// EdDSA).
// ... and, for the same entries, membership in a ClaimSet (jg_claims_match_set):
//   InSet         v is a string equal to a member of `set`
//   AnyElementIn  v is an array and one of its direct elements is a string equal
//                 to a member of `set` (HasElement's rules)
// At most 4 distinct resident sets are scanned per call; a call that names more,
// or a host-only set, is answered from the host path for every token.
// The numbers are jg_pred_op's (include/jg.h).
struct Require {
  enum Op : uint8_t {
    Equals = 1, HasWord = 2, HasElement = 3, Present = 4,
    EqualsArg = 5, AtLeast = 6, AtMost = 7, AtLeastArg = 8, AtMostArg = 9,
    HashOfArg = 10, IsString = 11, InSet = 12, AnyElementIn = 13
  };
  ClaimPath path;
  Op op = Present;
  std::string value;
  int64_t bound = 0;
  uint32_t column = 0;
  ClaimSet set{};                   // InSet, AnyElementIn
};
// One hash column of a MatchBatchArgs call: per token the value to hash (an
// access token, an authorization code: any bytes), or nothing
using HashColumn = std::vector<std::optional<std::string_view>>;
// At most this many per call: the mask has one bit per requirement (JG_MAX_PRED)
constexpr size_t kMaxRequires = 16;
// CheckBatch's (ok, error string) and, for an accepted token, bit k set when
// requires[k] holds on its claims.  A rejected token carries no bits.
struct MatchResult {
  bool ok = false;
  std::string err;
  uint32_t bits = 0;
};
// SelectBatch as columns (SelectBlob): RegisteredColumns plus, per name, the
// value's type, its number and its text.  Rows of a rejected token are empty.
struct SelectColumns {
  RegisteredColumns reg;
  struct Name {
    uint8_t* type = nullptr;        // n bytes of jg_sel_type (include/jg.h); a token the host path decided
                                    // reports JG_SEL_STRING for any string
    double* num = nullptr;          // n float64: the JG_SEL_NUMBER's value, else 0
    uint32_t* text_off = nullptr;   // n + 1 offsets into the name's text column
  };
  std::vector<Name> names;          // one per name, in the caller's order
  // The text column of name k, sized by the call: a string's UTF-8 bytes, or
  // json::marshal(value) for an array or an object (on both paths, so the bytes
  // do not depend on which path decided); empty for every other type.  Called
  // once per name, from the calling thread.
  std::function<void*(size_t k, size_t bytes)> alloc_text;
};

class Validator {
 public:
  explicit Validator(KeySet* ks) : ks_(ks) {}
  // A ClaimSet on this validator's key set (its device context).  Throws
  // std::invalid_argument for a NUL in a member and std::runtime_error for a 17th
  // live set or a failed load.  seed: random unless given (tests).
  ClaimSet NewClaimSet(const std::vector<std::string>& members, std::optional<uint32_t> seed = std::nullopt);
  Result Validate(std::string_view token, const Expected& expected);
  Results ValidateBatch(const std::vector<std::string_view>& tokens, const Expected& expected);
  // Verdict-only ValidateBatch: out[i] is Validate(tokens[i], expected)'s (ok,
  // error string), token for token, and no claims map is built for a token
  // whose registered claims the device decides.  Parse and signatures as
  // ValidateBatch; the payload segments are scanned on the GPU
  // (jg_claims_scan) while the signature batch is on the device; the alg
  // header check stays on the host.  A token the scan leaves to the host
  // (JG_CL_HOST, b64:false, a re-encoded token) takes today's path alone.
  std::vector<CheckResult> CheckBatch(const std::vector<std::string_view>& tokens, const Expected& expected,
                                      CheckStats* stats = nullptr);
  // CheckBatch's accept bits alone (1 = Validate returns no error): no error
  // string outlives the call (CheckBlob)
  std::vector<uint8_t> CheckVerdicts(const std::vector<std::string_view>& tokens, const Expected& expected,
                                     CheckStats* stats = nullptr);
  // CheckBatch plus what nearly every caller reads after a successful Validate:
  // ok / err are CheckBatch's, token for token, and an accepted token carries its
  // jwt.Claims.  The scan returns the values with the verdict
  // (jg_claims_extract): the dates as numbers, the strings as spans of the
  // decoded payload that a few bytes of base64 decoding turn into the value --
  // no JSON parse, no claims map.  A token the scan leaves to the host takes
  // the struct validate_claims decodes.
  std::vector<RegisteredResult> RegisteredBatch(const std::vector<std::string_view>& tokens, const Expected& expected,
                                                CheckStats* stats = nullptr);
  // RegisteredBatch's accept bits and claims as columns, built by the host
  // threads that merge the scan's records (RegisteredBlob)
  void RegisteredCols(const std::vector<std::string_view>& tokens, const Expected& expected,
                      const RegisteredColumns& out, CheckStats* stats = nullptr);
  // RegisteredBatch plus top-level claims outside the registered seven, by name
  // (scope, roles, tenant, nonce, azp, auth_time, ...): ok / err / claims are
  // RegisteredBatch's, token for token, and values[k] of an accepted token is
  // ValidateBatch's claims-map entry under names[k], exactly (case-sensitive).
  // The scan latches where each named member's value lies (jg_claims_select); a
  // string is cut out of the decoded payload, a number, array or object is
  // parsed from its own few bytes -- no claims map.  A token the scan leaves to
  // the host reads its verified claims map.  A name list the scan does not take
  // (more than JG_MAX_SELECT distinct names, a name that is empty, over
  // JG_SELECT_NAME_MAX bytes, or holds a quote, a backslash or a byte outside
  // printable ASCII) sends every token to the host path; equal names share a
  // slot.  Throws std::invalid_argument for a name with a NUL byte.
  std::vector<SelectResult> SelectBatch(const std::vector<std::string_view>& tokens, const Expected& expected,
                                        const std::vector<std::string>& names, CheckStats* stats = nullptr);
  // SelectBatch as columns, built by the host threads that merge the scan's
  // records (SelectBlob); out.names.size() == names.size()
  void SelectCols(const std::vector<std::string_view>& tokens, const Expected& expected,
                  const std::vector<std::string>& names, const SelectColumns& out, CheckStats* stats = nullptr);
  // The six entries above with an Expected per token, as Validate takes its
  // Expected per call: token i is held to expected[which[i]] -- its issuer,
  // audiences, subject, ID, SigningAlgorithms, Now (a profile without one reads
  // the wall clock, once per call) and leeways -- and its result is exactly what
  // the entry above returns for tokens[i] alone with that Expected.  One
  // signature submission and one scan (jg_claims_each) for the whole batch,
  // where a caller had to split it by tenant.  The scan's table holds
  // JG_MAX_PROFILES profiles and JG_PROFILE_POOL_BYTES of expected strings;
  // tokens of a profile beyond that, or of one the scan does not take, go the
  // host path, so results do not depend on the caps.  std::invalid_argument:
  // which.size() != tokens.size(), a which[i] >= expected.size(), no Expected
  // with tokens.
  std::vector<CheckResult> CheckBatchEach(const std::vector<std::string_view>& tokens,
                                          const std::vector<Expected>& expected, const std::vector<uint32_t>& which,
                                          CheckStats* stats = nullptr);
  std::vector<uint8_t> CheckVerdictsEach(const std::vector<std::string_view>& tokens,
                                         const std::vector<Expected>& expected, const std::vector<uint32_t>& which,
                                         CheckStats* stats = nullptr);
  std::vector<RegisteredResult> RegisteredBatchEach(const std::vector<std::string_view>& tokens,
                                                    const std::vector<Expected>& expected,
                                                    const std::vector<uint32_t>& which, CheckStats* stats = nullptr);
  void RegisteredColsEach(const std::vector<std::string_view>& tokens, const std::vector<Expected>& expected,
                          const std::vector<uint32_t>& which, const RegisteredColumns& out,
                          CheckStats* stats = nullptr);
  std::vector<SelectResult> SelectBatchEach(const std::vector<std::string_view>& tokens,
                                            const std::vector<Expected>& expected, const std::vector<uint32_t>& which,
                                            const std::vector<std::string>& names, CheckStats* stats = nullptr);
  void SelectColsEach(const std::vector<std::string_view>& tokens, const std::vector<Expected>& expected,
                      const std::vector<uint32_t>& which, const std::vector<std::string>& names,
                      const SelectColumns& out, CheckStats* stats = nullptr);
  // The four Select entries for claims inside objects: values[k] (column set
  // k) is what walking ValidateBatch's claims map along paths[k] reaches -- at
  // each component the current value must be an object and hold the key, else
  // the claim is absent; arrays are never descended.  A one-component path is
  // the name.  The scan matches component j against the keys at depth j of the
  // object that components 1..j-1 opened (jg_claims_paths) and latches the value
  // as for a name; a token the scan leaves to the host walks its verified claims
  // map.  A path list the scan does not take (more than JG_MAX_PATHS distinct
  // paths, a path of more than JG_PATH_MAX_COMP components, a component a name
  // list would not be taken for) sends every token to the host path; equal paths
  // share a slot.  Throws std::invalid_argument for a path without components
  // and for a component with a NUL byte.
  std::vector<SelectResult> SelectBatch(const std::vector<std::string_view>& tokens, const Expected& expected,
                                        const ClaimPaths& paths, CheckStats* stats = nullptr);
  void SelectCols(const std::vector<std::string_view>& tokens, const Expected& expected,
                  const ClaimPaths& paths, const SelectColumns& out, CheckStats* stats = nullptr);
  std::vector<SelectResult> SelectBatchEach(const std::vector<std::string_view>& tokens,
                                            const std::vector<Expected>& expected, const std::vector<uint32_t>& which,
                                            const ClaimPaths& paths, CheckStats* stats = nullptr);
  void SelectColsEach(const std::vector<std::string_view>& tokens, const std::vector<Expected>& expected,
                      const std::vector<uint32_t>& which, const ClaimPaths& paths,
                      const SelectColumns& out, CheckStats* stats = nullptr);
  // CheckBatch plus yes/no questions about claims, answered where the bytes are:
  // ok / err are CheckBatch's, token for token, and bit k of an accepted token's
  // bits says whether requires[k] holds on ValidateBatch's claims map for it (the
  // value reached as the Select entries' paths reach it).  The scan compares the
  // values while it walks the payload (jg_claims_match) and returns four bytes per
  // token: no span, no merge of text, no column.  A requirement never changes ok
  // or err.  A token the scan leaves to the host evaluates the same requirements
  // on its verified claims map (match_requires).  A list the scan does not take
  // (more than JG_MAX_PATHS distinct paths, a path of more than JG_PATH_MAX_COMP
  // components, a component or a value with a byte it refuses, a value over
  // JG_PRED_VALUE_MAX bytes, an empty value or one with a space for HasWord, an
  // empty value for HasElement) sends every token to the host path, so results do
  // not depend on the caps; equal requirements are scanned once.  Throws
  // std::invalid_argument for more than kMaxRequires requirements, a path without
  // components, a component or a value with a NUL byte, and an unknown op.
  std::vector<MatchResult> MatchBatch(const std::vector<std::string_view>& tokens, const Expected& expected,
                                      const std::vector<Require>& requires_, CheckStats* stats = nullptr);
  // MatchBatch's accept bits and masks alone (MatchBlob): ok[i] is 1 when Validate
  // returns no error, bits[i] the mask (0 for a rejected token); n entries each
  void MatchVerdicts(const std::vector<std::string_view>& tokens, const Expected& expected,
                     const std::vector<Require>& requires_, uint8_t* ok, uint32_t* bits, CheckStats* stats = nullptr);
  // ... and with an Expected per token, as the *Each entries above
  std::vector<MatchResult> MatchBatchEach(const std::vector<std::string_view>& tokens,
                                          const std::vector<Expected>& expected, const std::vector<uint32_t>& which,
                                          const std::vector<Require>& requires_, CheckStats* stats = nullptr);
  void MatchVerdictsEach(const std::vector<std::string_view>& tokens, const std::vector<Expected>& expected,
                         const std::vector<uint32_t>& which, const std::vector<Require>& requires_, uint8_t* ok,
                         uint32_t* bits, CheckStats* stats = nullptr);
  // MatchBatch for the checks whose other side differs from token to token (the
  // nonce of that request, auth_time under its max_age, sub against the session's
  // subject): `strs` holds the string columns and `nums` the number columns, each
  // with one entry per token, and a requirement may be EqualsArg, AtLeast, AtMost,
  // AtLeastArg or AtMostArg (jg_claims_match_args).  The device decides a numeric
  // requirement on an integer literal of at most 15 digits; a token whose number
  // is written otherwise (a fraction, more digits) is left to the host path, which
  // compares the float64 as Go does.  A token whose own string operand the scan
  // does not take (a byte outside 0x20..0x7e, a quote, a backslash, over
  // JG_PRED_VALUE_MAX bytes) takes the host path too; a list over the scan's caps
  // (MatchBatch's, or more than JG_MAX_ARGS columns of a kind) sends every token
  // there.  Results never depend on the caps.  Throws std::invalid_argument for
  // what MatchBatch throws for (an unknown op is one outside 1..9), a column whose
  // length is not the number of tokens, a column index without a column, and a
  // NUL byte in an operand.
  // `hashes` holds the hash columns, each with one entry per token, for HashOfArg;
  // IsString needs none.  A call with a hash column or one of these two ops goes
  // through jg_claims_match_hash: the values are uploaded beside the tokens and
  // hashed and encoded on the device, in front of the scan.  A token whose value is
  // over JG_HASH_SRC_MAX bytes takes the host path, as do the tokens the scan
  // leaves to it; there the digests come from one jg_hash_batch call over just
  // those tokens' values.  More than JG_MAX_HASH_ARGS hash columns, or more than
  // JG_MAX_ARGS string and hash columns together, send every token to the host
  // path.  Throws also for a hash column whose length is not the number of tokens
  // and a hash column index without a column; here an unknown op is one outside
  // 1..11.
  std::vector<MatchResult> MatchBatchArgs(const std::vector<std::string_view>& tokens, const Expected& expected,
                                          const std::vector<Require>& requires_,
                                          const std::vector<std::vector<std::string_view>>& strs,
                                          const std::vector<const int64_t*>& nums, CheckStats* stats = nullptr,
                                          const std::vector<HashColumn>& hashes = {});
  void MatchVerdictsArgs(const std::vector<std::string_view>& tokens, const Expected& expected,
                         const std::vector<Require>& requires_, const std::vector<std::vector<std::string_view>>& strs,
                         const std::vector<const int64_t*>& nums, uint8_t* ok, uint32_t* bits,
                         CheckStats* stats = nullptr, const std::vector<HashColumn>& hashes = {});
  std::vector<MatchResult> MatchBatchArgsEach(const std::vector<std::string_view>& tokens,
                                              const std::vector<Expected>& expected, const std::vector<uint32_t>& which,
                                              const std::vector<Require>& requires_,
                                              const std::vector<std::vector<std::string_view>>& strs,
                                              const std::vector<const int64_t*>& nums, CheckStats* stats = nullptr,
                                          const std::vector<HashColumn>& hashes = {});
  void MatchVerdictsArgsEach(const std::vector<std::string_view>& tokens, const std::vector<Expected>& expected,
                             const std::vector<uint32_t>& which, const std::vector<Require>& requires_,
                             const std::vector<std::vector<std::string_view>>& strs,
                             const std::vector<const int64_t*>& nums, uint8_t* ok, uint32_t* bits,
                             CheckStats* stats = nullptr, const std::vector<HashColumn>& hashes = {});
 private:
  KeySet* ks_;
};
// nil keySet -> error "keySet must not be nil"
std::unique_ptr<Validator> NewValidator(KeySet* ks, std::string* err);

// The claim checks of Validate after the signature (jwt/jwt.go:103-201), on a
// verified claims map and the token's parse info.  Exposed for tests.
Result validate_claims(const json::Value& all_claims, const TokenInfo& info, const Expected& expected,
                       int64_t now_unix_ns);
Result validate_claims(const json::Value& all_claims, const TokenView& info, const Expected& expected,
                       int64_t now_unix_ns);
// ... and *decoded = the jwt.Claims struct the checks ran on (set once the
// claims map unmarshals, whatever the checks then say)
Result validate_claims(const json::Value& all_claims, const TokenView& info, const Expected& expected,
                       int64_t now_unix_ns, RegisteredClaims* decoded);
// The requirements of a MatchBatch call on a verified claims map: bit k set
// when requires[k] holds.  What the host path of MatchBatch runs; exposed for
// tests.  Throws as MatchBatch does.
uint32_t match_requires(const json::Value& all_claims, const std::vector<Require>& requires_);
// ... and of a MatchBatchArgs call with one token's operands: strs[c] and nums[c]
// are its entries in column c.  What the host path of MatchBatchArgs runs.
uint32_t match_requires(const json::Value& all_claims, const std::vector<Require>& requires_,
                        const std::vector<std::string_view>& strs, const std::vector<int64_t>& nums);
// ... and with one token's hash columns, already hashed: hashed[c] is
// base64.RawURLEncoding(SHA-2(value)[:size/2]) of its entry in hash column c, or
// nothing (an absent entry, EdDSA).  Takes HashOfArg and IsString too.
uint32_t match_requires(const json::Value& all_claims, const std::vector<Require>& requires_,
                        const std::vector<std::string_view>& strs, const std::vector<int64_t>& nums,
                        const std::vector<std::optional<std::string>>& hashed);
// The value a hash claim must equal: base64.RawURLEncoding of the left half of a
// digest (32, 48 or 64 bytes).  What the host path makes of jg_hash_batch's output.
std::string hash_claim_value(const uint8_t* digest, int fam);
// Expected's three leeways after Go's defaulting (jwt/jwt.go:128-170): the
// clock skew in ns (negative -> 0, 0 -> one minute) and the leeways that
// default a missing exp / nbf, as the whole seconds Go adds (negative -> 0,
// 0 -> 150 s, then int64(float64 seconds)).  validate_claims and the claims
// scan's resolved Expected share it.
struct Leeways {
  int64_t skew_ns = 0, exp_s = 0, nbf_s = 0;
};
Leeways resolve_leeways(const Expected& expected);

bool ParsePublicKeyPEM(std::string_view data, PublicKey* out, std::string* err);

// Frees a batch's results now (all host threads; the destructor does the same).
void release_results(Results& rs);

// Host threads used by batch parsing / claims (CAPJWT_HOST_THREADS, default
// available_cpus()): declared above.
// CPUs available to this process (affinity mask, cgroup v2 quota)
int available_cpus();

// ---------------------------------------------------------------- oidc hash claims
// IDToken.VerifyAccessToken / VerifyAuthorizationCode (oidc/id_token.go:59-145,
// verifyHashClaim) for many (id_token, value) pairs: claims via UnmarshalClaims
// (oidc/token.go:170-184), the claim as a string, jose.ParseSigned, exactly one
// signature with a supported alg, then base64url(left half of SHA-2(value)) ==
// claim.  The SHA-2 runs on the GPU in one jg_hash_batch.  verified/err are Go's
// (bool, error); err == "" <=> nil.  Error strings follow the reference,
// including its "VerifyAccessToken" op prefix on the c_hash path.
struct HashClaimResult {
  bool verified = false;
  std::string err;
};
std::vector<HashClaimResult> VerifyAccessTokenBatch(Engine& eng, const std::vector<std::string_view>& id_tokens,
                                                    const std::vector<std::string_view>& access_tokens);
std::vector<HashClaimResult> VerifyAuthorizationCodeBatch(Engine& eng, const std::vector<std::string_view>& id_tokens,
                                                          const std::vector<std::string_view>& codes);

}  // namespace capjwt
