// ratelimiter.hpp — C++ mirror of the reference's Java API over the C-ABI engine.
//
// The reference (Java 17) API this mirrors, name for name:
//   com.ratelimiter.core.RateLimiter            core/RateLimiter.java:7-44
//   com.ratelimiter.core.RateLimitConfig        core/RateLimitConfig.java:12-81
//   com.ratelimiter.storage.StorageException    storage/StorageException.java:6-14
//   SlidingWindowRateLimiter / TokenBucketRateLimiter constructors and argument checks
//                                               algorithms/SlidingWindowRateLimiter.java:46-131
//                                               algorithms/TokenBucketRateLimiter.java:70-116
// Java's toolchain is not available in this build, so the host side above the C-ABI is
// C++ (INTEGRATION.md shows the JNI binding a Java maintainer adds instead). Every
// decision is made on the GPU through include/rl_engine.h; nothing here computes one.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <string_view>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/rl_engine.h"

namespace ratelimiter {

// java.lang.IllegalArgumentException
struct IllegalArgumentException : std::invalid_argument {
    using std::invalid_argument::invalid_argument;
};

// com.ratelimiter.storage.StorageException (unchecked; thrown on backend failure,
// RedisRateLimitStorage.java:177) — here: a HIP/device error from the engine.
struct StorageException : std::runtime_error {
    int status;
    StorageException(const std::string& m, int st) : std::runtime_error(m), status(st) {}
};

// RateLimitConfig (RateLimitConfig.java:12-81). Immutable value; Duration fields are
// milliseconds here.
struct RateLimitConfig {
    int64_t maxPermits = 0;
    int64_t windowMs = 0;
    double refillRate = 0.0;          // permits per second (token bucket only)
    bool enableLocalCache = true;     // @Builder.Default true (RateLimitConfig.java:37-38)
    int64_t localCacheTtlMs = 100;    // @Builder.Default 100 ms (:43-44)
    uint64_t expectedKeys = 0;        // engine table sizing (not in the reference)

    // validate() (RateLimitConfig.java:46-56)
    void validate() const {
        if (maxPermits <= 0) throw IllegalArgumentException("maxPermits must be positive");
        if (windowMs <= 0) throw IllegalArgumentException("window must be a positive duration");
        if (refillRate < 0) throw IllegalArgumentException("refillRate cannot be negative");
    }
    // factories (RateLimitConfig.java:61-80)
    static RateLimitConfig perSecond(int64_t maxPermits) { return make(maxPermits, 1000); }
    static RateLimitConfig perMinute(int64_t maxPermits) { return make(maxPermits, 60000); }
    static RateLimitConfig perHour(int64_t maxPermits) { return make(maxPermits, 3600000); }

  private:
    static RateLimitConfig make(int64_t m, int64_t w) {
        RateLimitConfig c;
        c.maxPermits = m;
        c.windowMs = w;
        return c;
    }
};

// RateLimiter (RateLimiter.java:7-44).
class RateLimiter {
  public:
    virtual ~RateLimiter() = default;
    virtual bool tryAcquire(const std::string& key) = 0;               // :16
    virtual bool tryAcquire(const std::string& key, int permits) = 0;  // :26
    virtual int64_t getAvailablePermits(const std::string& key) = 0;   // :35 (-1 if unknown)
    virtual void reset(const std::string& key) = 0;                    // :43
};

// The four numbers of a response's rate-limit headers (the reference's API_EXAMPLES.md:205-213):
// X-RateLimit-Limit, X-RateLimit-Remaining, X-RateLimit-Reset and the 429's Retry-After, the
// last two as milliseconds from the query's now.
struct RateLimitQuota {
    int64_t limit;              // the configured maxPermits
    int64_t remaining;          // getAvailablePermits
    int64_t resetMillis;        // until getAvailablePermits reads `limit` again (0: it does now)
    int64_t retryAfterMillis;   // until tryAcquire(key, permits) would be allowed (-1: never)
};

// Micrometer counter stand-ins with the reference's meter names
// (SlidingWindowRateLimiter.java:67-77, TokenBucketRateLimiter.java:87-93).
struct Counter {
    std::string name;
    std::atomic<uint64_t> value{0};
    explicit Counter(std::string n) : name(std::move(n)) {}
    void increment(uint64_t d = 1) { value.fetch_add(d, std::memory_order_relaxed); }
    uint64_t count() const { return value.load(std::memory_order_relaxed); }
};

// String -> 64-bit key hash (build-defined): FNV-1a over the UTF-8
// bytes followed by the splitmix64 finaliser. Collisions between distinct strings make
// them share state (probability ~ n^2 / 2^65). One definition: rl_key_hash (rl_engine.h).
uint64_t keyHash(const std::string& key);

// A batch of string keys in the layout of rl_hash_keys / rl_execute_batch_keys: the keys' UTF-8
// bytes back to back plus size() + 1 offsets. add() throws IllegalArgumentException for a key
// longer than RL_KEY_MAX_BYTES (the per-call tryAcquire(String) path has no such limit).
class KeyBatch {
  public:
    void add(std::string_view key);
    size_t size() const { return off_.size() - 1; }
    const std::vector<uint8_t>& bytes() const { return bytes_; }
    const std::vector<uint64_t>& offsets() const { return off_; }
    void clear() { bytes_.clear(); off_.assign(1, 0); }

  private:
    std::vector<uint8_t> bytes_;
    std::vector<uint64_t> off_ = std::vector<uint64_t>(1, 0);
};

// One GPU engine (rl_create). Thread-safe: the engine serialises batches.
class GpuEngine {
  public:
    struct Options {
        int device = 0;
        uint64_t maxBatch = 1u << 20;
        uint64_t defaultCapacity = 1u << 20;
        int64_t maxSkewMs = 0;          // rl_opts.max_skew_ms
    };
    explicit GpuEngine(const Options& o);
    GpuEngine() : GpuEngine(Options{}) {}
    ~GpuEngine();
    GpuEngine(const GpuEngine&) = delete;
    GpuEngine& operator=(const GpuEngine&) = delete;
    rl_engine* handle() const { return e_; }
    // Page-lock a reused host buffer for the engine's DMA (rl_pin_host); best effort:
    // an unpinned buffer still works through pageable staging.
    void pin(void* p, size_t bytes) { if (p && bytes) (void)rl_pin_host(e_, p, bytes); }
    void unpin(void* p) { if (p) (void)rl_unpin_host(e_, p); }
    uint16_t addLimiter(int algo, const RateLimitConfig& c);
    // Runs one host batch and returns its status and cache-hit count atomically with
    // respect to the other limiters sharing this engine.
    int executeBatch(size_t n, const uint64_t* key, const int32_t* permits, const int64_t* now,
                     const uint16_t* limiter, const uint8_t* op, uint8_t* allowed,
                     int64_t* remaining, uint64_t* cacheHits);
    // rl_execute_batch_keys: the same batch on string keys, hashed on the device; keyHashOut
    // (nullable) receives keyHash of every key.
    int executeBatchKeys(const KeyBatch& keys, const int32_t* permits, const int64_t* now,
                         const uint16_t* limiter, const uint8_t* op, uint8_t* allowed,
                         int64_t* remaining, uint64_t* keyHashOut, uint64_t* cacheHits);
    // rl_hash_keys: keyHash of every key of the batch, computed on the device (read-only).
    std::vector<uint64_t> hashKeys(const KeyBatch& keys);
    // rl_retry_after: ms until an acquire would be allowed (read-only; skip nullable).
    int retryAfter(size_t n, const uint64_t* key, const int32_t* permits, const int64_t* now,
                   const uint16_t* limiter, const uint8_t* skip, int64_t* waitMs);
    // rl_quota: per query what getAvailablePermits reads at now, the ms until it reads maxPermits
    // again and, with permits and retryMs (given together; skip only with them), the retryAfter
    // wait, from one lookup per key (read-only; limiter nullable).
    int quota(size_t n, const uint64_t* key, const int64_t* now, const uint16_t* limiter,
              const int32_t* permits, const uint8_t* skip, int64_t* remaining, int64_t* resetMs,
              int64_t* retryMs);
    // rl_top_keys: the (key hash, count) pairs of the at most k most frequent of the hashes
    // that occur at least minCount times, count descending then hash ascending; exact.
    // Throws StorageException when the sample overflows the engine's candidate store
    // (RL_E_CAPACITY), IllegalArgumentException for k == 0, k > RL_TOP_KEYS_MAX, minCount == 0.
    std::vector<std::pair<uint64_t, uint64_t>> topKeys(const uint64_t* hashes, size_t n, uint32_t k,
                                                       uint64_t minCount);
    // rl_tally_batch: the per-limiter counts of a finished batch (its submitted permits / limiter /
    // op and its answered allowed / remaining; limiter and op nullable), as (row, tally) pairs of
    // the rows with requests > 0 in ascending row order; row RL_TALLY_UNKNOWN collects the
    // requests under ids this engine does not know. A row's tally.allowed / tally.denied are the
    // reference's meters for that limiter and batch: ratelimiter.requests.allowed / .rejected
    // for a sliding window (SlidingWindowRateLimiter.java:67-77), ratelimiter.tokenbucket.allowed
    // / .rejected for a token bucket (TokenBucketRateLimiter.java:87-93; over_max, its
    // permits > maxPermits rejections of :114, is part of denied). Read-only.
    std::vector<std::pair<uint16_t, rl_limiter_tally>> tallyBatch(size_t n, const int32_t* permits,
                                                                  const uint16_t* limiter, const uint8_t* op,
                                                                  const uint8_t* allowed,
                                                                  const int64_t* remaining);
    // rl_top_denied: the (key hash, denials) pairs of the at most k keys most often denied under
    // `limiter` in a finished batch, among those denied at least minCount times; order and
    // exceptions as topKeys. nDenied (nullable) = the batch's denials under that limiter.
    std::vector<std::pair<uint64_t, uint64_t>> topDenied(size_t n, const uint64_t* hashes, const int32_t* permits,
                                                         const uint16_t* limiterIds, const uint8_t* op,
                                                         const uint8_t* allowed, const int64_t* remaining,
                                                         uint16_t limiter, uint32_t k, uint64_t minCount,
                                                         uint64_t* nDenied = nullptr);
    // rl_limiter_usage: census of a limiter's table at nowNanos (read-only).
    rl_usage usage(uint16_t limiter, int64_t nowNanos);
    // rl_top_consumers: the (key hash, used permits) pairs of the at most k live keys of the
    // limiter that have used at least minUsed permits at nowNanos, used descending then hash
    // ascending; exact however many keys tie. nMatch (nullable) = how many keys qualify.
    // IllegalArgumentException for k == 0, k > RL_TOP_KEYS_MAX, minUsed < 0.
    std::vector<std::pair<uint64_t, int64_t>> topConsumers(uint16_t limiter, int64_t nowNanos, uint32_t k,
                                                           int64_t minUsed, uint64_t* nMatch = nullptr);
    // rl_snapshot_keys over a limiter's whole table: `sink` receives the images chunk by chunk (at
    // most chunkImages each, at least RL_SNAPSHOT_MIN_CAP), in (region, slot) order; the chunks
    // together are a point-in-time checkpoint if no batch runs on this engine meanwhile (the engine
    // is held for the whole call, so none of this object's does). Returns the images delivered.
    // Read-only. IllegalArgumentException for an unknown limiter, StorageException if the table
    // grew between two chunks (RL_E_INTERNAL) or on a device error.
    using SnapshotSink = std::function<void(const rl_key_image*, size_t)>;
    size_t snapshot(uint16_t limiter, size_t chunkImages, const SnapshotSink& sink);
    // rl_restore_keys: puts images (a snapshot's chunks in order take the device's ordered path,
    // anything else the path of rl_put_keys) into this engine's tables as they are sized; size a
    // fresh engine's limiter first (RateLimitConfig.expectedKeys, or rl_grow_limiter). Returns the
    // images put; StorageException with RL_E_CAPACITY if a region had no free slot.
    size_t restore(const rl_key_image* images, size_t n);
    // rl_shrink_limiter: halves the limiter's region count as often as its keys live at nowNanos
    // allow (room for minKeys keys is kept), dropping dead slots on the way; returns the plan acted
    // on (halvings == 0: the table was left alone). Decisions are unchanged. nowNanos must not
    // exceed the now of any later request. IllegalArgumentException for an unknown limiter,
    // StorageException on a device error (the old table then still stands).
    rl_shrink_report shrink(uint16_t limiter, int64_t nowNanos, uint64_t minKeys = 0);
    // rl_limiter_digest: the 2^bucketBits per-bucket fingerprints of the limiter's live state at
    // nowNanos (with the rejecting local-cache entries unless withCache is false). Equal digests =
    // the same Redis keyspace, whatever the tables' sizes. Read-only. IllegalArgumentException for
    // an unknown limiter or bucketBits beyond the table's region bits.
    std::vector<rl_bucket_digest> digest(uint16_t limiter, int64_t nowNanos, uint32_t bucketBits,
                                         bool withCache = true);
    // Incremental checkpoint: computes the digests (with cache entries) into *current (nullable)
    // and, for every bucket whose digest differs from `previous` (empty: every bucket), delivers
    // the bucket's images through rl_snapshot_keys over its region range, in chunks of at most
    // chunkImages (at least RL_SNAPSHOT_MIN_CAP). `sink` is called at least once per changed
    // bucket, with n == 0 if the bucket holds nothing now, so a checkpoint store replaces that
    // bucket's chunk wholesale; an unchanged bucket is never delivered. Returns the images
    // delivered. The engine is held for the whole call, as by snapshot(). Throws as snapshot():
    // IllegalArgumentException for an unknown limiter, bucketBits too large or a `previous` whose
    // length is not 2^bucketBits, StorageException if the table grew between two chunks.
    using BucketSink = std::function<void(uint32_t bucket, const rl_key_image*, size_t)>;
    size_t snapshotChanged(uint16_t limiter, int64_t nowNanos, uint32_t bucketBits,
                           const std::vector<rl_bucket_digest>& previous,
                           std::vector<rl_bucket_digest>* current, size_t chunkImages,
                           const BucketSink& sink);
    // rl_check_limiter over the limiter's whole table: how many slots break which of the slot
    // invariants, and where the first one is (bad_slots == 0: the table is sound). What
    // redis-check-rdb answers for the reference's Redis; call it after a restore, a migration or
    // an RL_E_INTERNAL. Read-only. IllegalArgumentException for an unknown limiter.
    rl_check_report check(uint16_t limiter);
    // rl_check_images: the value classes over images before they are restored (first[] holds
    // image indices). Read-only.
    rl_check_report checkImages(const rl_key_image* images, size_t n);
    // rl_tune "small_batch": host and device batches of at most min(n, RL_SMALL_BATCH_MAX) requests
    // are decided by one kernel launch and one round trip (rl_engine.h, "small batches"); 0 turns
    // the path off. The same decisions either way. Returns the status code.
    int setSmallBatch(uint64_t n);
    // rl_small_batches: {taken, declined} since the engine was created.
    std::pair<uint64_t, uint64_t> smallBatches();

  private:
    rl_engine* e_ = nullptr;
    std::mutex mu_;
};

// Clock in nanoseconds (the reference reads System.currentTimeMillis(); injectable so a
// trace can be replayed with a pinned clock).
using Clock = std::function<int64_t()>;
int64_t systemNanos();

// Drop-in GPU implementation of RateLimiter for one limiter configuration. The
// constructor performs the reference constructors' checks; single calls are batched by
// a micro-batcher (concurrent callers share one engine batch, arrival order = the order
// in which callers enter the queue).
class GpuRateLimiter : public RateLimiter {
  public:
    enum class Algorithm { SlidingWindow = RL_ALGO_SLIDING_WINDOW, TokenBucket = RL_ALGO_TOKEN_BUCKET };

    // smallBatch > 0: the micro-batcher's flushes, getAvailablePermits and reset of up to that
    // many requests take the engine's small-batch path (GpuEngine::setSmallBatch; the setting is
    // the engine's, so it holds for every limiter sharing it, and the last setting wins); 0 leaves
    // the engine as it is. kSmallBatchDefault is the measured crossover (DESIGN.md §4 "Small
    // batches"): the largest measured batch the path still answers sooner than the pipeline
    // (n = 1: 33 us against 305 us per call; n = 256: 227 us against 302 us).
    static constexpr uint64_t kSmallBatchDefault = 256;
    GpuRateLimiter(std::shared_ptr<GpuEngine> engine, Algorithm algo, const RateLimitConfig& cfg,
                   Clock clock = systemNanos, int batchWindowMicros = 0,
                   uint64_t smallBatch = kSmallBatchDefault);
    ~GpuRateLimiter() override;

    bool tryAcquire(const std::string& key) override { return tryAcquire(key, 1); }
    bool tryAcquire(const std::string& key, int permits) override;
    int64_t getAvailablePermits(const std::string& key) override;
    void reset(const std::string& key) override;

    // Milliseconds, from the clock's now, until tryAcquire(key, permits) would be allowed on the
    // key's state as it stands (0: now; -1: never, permits > maxPermits): what a caller puts
    // into Retry-After beside a 429 (the reference's DemoController.rateLimitExceeded). It is
    // not X-RateLimit-Reset: that is about maxPermits and does not count the local cache
    // (quota().resetMillis). Not part of the reference's RateLimiter interface.
    // Read-only; it sees every tryAcquire of this object that has returned.
    int64_t retryAfterMillis(const std::string& key, int permits = 1);
    // Every rate-limit header of one response from one lookup at the clock's now: limit (the
    // config's maxPermits), remaining (= getAvailablePermits), resetMillis and retryAfterMillis
    // (= retryAfterMillis(key, permits)). Throws IllegalArgumentException for permits <= 0.
    // Read-only; it sees every tryAcquire of this object that has returned.
    RateLimitQuota quota(const std::string& key, int permits = 1);
    // What is in this limiter's table at the clock's now (DBSIZE / INFO keyspace of the
    // reference's Redis; the numbers behind /api/health): slots, live and throttled keys, permits
    // in use. Read-only; sees every tryAcquire of this object that has returned.
    rl_usage usage();
    // The at most k live keys that have used at least minUsed permits, heaviest first, as
    // (keyHash(key), used) pairs (the candidates for reset(key) or an abuse report). Exact.
    // Throws IllegalArgumentException for k == 0, k > RL_TOP_KEYS_MAX, minUsed < 0.
    std::vector<std::pair<uint64_t, int64_t>> topConsumers(uint32_t k, int64_t minUsed = 1);
    // Gives this limiter's table memory back after a flood of keys has expired (Redis frees
    // memory as keys expire): shrinks its own table at the clock's now, as usage() reads it, and
    // keeps room for config().expectedKeys. Sees every tryAcquire of this object that has
    // returned; later decisions are unchanged.
    rl_shrink_report compact();
    // The 2^bucketBits per-bucket fingerprints of this limiter's state at the clock's now (with
    // its rejecting local-cache entries): compare with a replica's or a restored engine's, or
    // keep them for GpuEngine::snapshotChanged. Read-only; sees every tryAcquire that has returned.
    std::vector<rl_bucket_digest> digest(uint32_t bucketBits);
    // Is this limiter's table sound (GpuEngine::check)? Read-only; sees every tryAcquire of this
    // object that has returned.
    rl_check_report check();
    // the reference's permits check (SlidingWindowRateLimiter.java:87-89,
    // TokenBucketRateLimiter.java:106-108): throws IllegalArgumentException for permits <= 0
    static void requirePositive(int permits);

    // tryAcquireBatch(keys[], permits[], nowNanos[]); remaining may be null.
    void tryAcquireBatch(size_t n, const uint64_t* keyHash, const int32_t* permits,
                         const int64_t* nowNanos, bool* allowed, int64_t* remaining);
    // The same on string keys (keys.size() requests), hashed on the device in the batch's own
    // submission: the decisions, counters and exceptions of the overload above on keyHash of
    // every key; keyHashOut (nullable) receives those hashes.
    void tryAcquireBatch(const KeyBatch& keys, const int32_t* permits, const int64_t* nowNanos,
                         bool* allowed, int64_t* remaining, uint64_t* keyHashOut = nullptr);

    uint16_t limiterId() const { return id_; }
    const RateLimitConfig& config() const { return cfg_; }
    Counter allowedRequests;
    Counter rejectedRequests;
    Counter cacheHits{"ratelimiter.cache.hits"};     // SlidingWindowRateLimiter.java:75-77

  private:
    struct Pending {
        uint64_t key;
        int32_t permits;
        int64_t now;
        uint8_t op;
        bool done = false;
        uint8_t allowed = 0;
        int64_t remaining = 0;
        int status = RL_OK;
    };
    void submit(Pending& p);
    void flushLocked(std::unique_lock<std::mutex>& lk);
    void checkStatus(int st, const char* where);
    // the body of both tryAcquireBatch overloads; run(limiter ids, allowed, remaining, cache hits)
    // makes the engine call
    using BatchCall = std::function<int(const uint16_t*, uint8_t*, int64_t*, uint64_t*)>;
    void acquireBatch(size_t n, const BatchCall& run, bool* allowed, int64_t* remaining);

    std::shared_ptr<GpuEngine> engine_;
    Algorithm algo_;
    RateLimitConfig cfg_;
    Clock clock_;
    uint16_t id_ = 0;
    int windowMicros_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<Pending*> queue_;
    bool flushing_ = false;
    // flush buffers, reused across flushes and page-locked (owned by the flush slot)
    struct FlushBufs {
        size_t cap = 0;
        std::vector<uint64_t> key;
        std::vector<int32_t> permits;
        std::vector<int64_t> now, remaining;
        std::vector<uint16_t> lim;
        std::vector<uint8_t> op, allowed;
    } fb_;
    void reserveFlush(size_t n);
    void unpinFlush();
};

}  // namespace ratelimiter
