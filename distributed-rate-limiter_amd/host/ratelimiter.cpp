// ratelimiter.cpp — see ratelimiter.hpp.
#include "ratelimiter.hpp"

#include <algorithm>
#include <cstring>

namespace ratelimiter {

uint64_t keyHash(const std::string& key) { return rl_key_hash(key.data(), key.size()); }

void KeyBatch::add(std::string_view key) {
    if (key.size() > RL_KEY_MAX_BYTES)
        throw IllegalArgumentException("KeyBatch: key longer than RL_KEY_MAX_BYTES");
    bytes_.insert(bytes_.end(), key.begin(), key.end());
    off_.push_back(bytes_.size());
}

int64_t systemNanos() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::system_clock::now().time_since_epoch())
        .count();
}

GpuEngine::GpuEngine(const Options& o) {
    rl_opts opts{};
    opts.device = o.device;
    opts.max_batch = o.maxBatch;
    opts.default_capacity = o.defaultCapacity;
    opts.shard_count = 1;
    opts.max_skew_ms = o.maxSkewMs;
    int st = rl_create(&opts, &e_);
    if (st != RL_OK) throw StorageException(std::string("rl_create: ") + rl_strerror(st), st);
}

GpuEngine::~GpuEngine() { rl_destroy(e_); }

uint16_t GpuEngine::addLimiter(int algo, const RateLimitConfig& c) {
    rl_limiter_config lc{};
    lc.algo = algo;
    lc.max_permits = c.maxPermits;
    lc.window_ms = c.windowMs;
    lc.refill_per_s = c.refillRate;
    lc.capacity = c.expectedKeys;
    if (algo == RL_ALGO_SLIDING_WINDOW && c.enableLocalCache && c.localCacheTtlMs > 0) {
        lc.flags = RL_LIM_LOCAL_CACHE;               // SlidingWindowRateLimiter.java:57-64
        lc.local_cache_ttl_ms = c.localCacheTtlMs;
    }
    uint16_t id = 0;
    int st = rl_add_limiter_ex(e_, &lc, &id);
    if (st == RL_E_INVALID_ARG)
        throw IllegalArgumentException(std::string("limiter configuration rejected: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("rl_add_limiter: ") + rl_strerror(st), st);
    return id;
}

int GpuEngine::executeBatch(size_t n, const uint64_t* key, const int32_t* permits,
                            const int64_t* now, const uint16_t* limiter, const uint8_t* op,
                            uint8_t* allowed, int64_t* remaining, uint64_t* cacheHits) {
    std::lock_guard<std::mutex> lk(mu_);
    const int st = rl_execute_batch(e_, n, key, permits, now, limiter, op, allowed, remaining, nullptr);
    rl_batch_stats bs{};
    if (cacheHits) *cacheHits = rl_batch_stats_get(e_, &bs) == RL_OK ? bs.cache_hits : 0;
    return st;
}

int GpuEngine::setSmallBatch(uint64_t n) {
    std::lock_guard<std::mutex> lk(mu_);
    return rl_tune(e_, "small_batch", (int64_t)std::min<uint64_t>(n, (uint64_t)INT64_MAX));
}

std::pair<uint64_t, uint64_t> GpuEngine::smallBatches() {
    std::lock_guard<std::mutex> lk(mu_);
    uint64_t taken = 0, declined = 0;
    (void)rl_small_batches(e_, &taken, &declined);
    return {taken, declined};
}

int GpuEngine::executeBatchKeys(const KeyBatch& keys, const int32_t* permits, const int64_t* now,
                                const uint16_t* limiter, const uint8_t* op, uint8_t* allowed,
                                int64_t* remaining, uint64_t* keyHashOut, uint64_t* cacheHits) {
    std::lock_guard<std::mutex> lk(mu_);
    const int st = rl_execute_batch_keys(e_, keys.size(), keys.bytes().data(), keys.bytes().size(),
                                         keys.offsets().data(), permits, now, limiter, op, allowed,
                                         remaining, nullptr, keyHashOut);
    rl_batch_stats bs{};
    if (cacheHits) *cacheHits = rl_batch_stats_get(e_, &bs) == RL_OK ? bs.cache_hits : 0;
    return st;
}

std::vector<uint64_t> GpuEngine::hashKeys(const KeyBatch& keys) {
    std::vector<uint64_t> out(keys.size());
    int st;
    {
        std::lock_guard<std::mutex> lk(mu_);
        st = rl_hash_keys(e_, keys.size(), keys.bytes().data(), keys.bytes().size(),
                          keys.offsets().data(), out.data());
    }
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("hashKeys: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("hashKeys: ") + rl_strerror(st), st);
    return out;
}

int GpuEngine::retryAfter(size_t n, const uint64_t* key, const int32_t* permits, const int64_t* now,
                          const uint16_t* limiter, const uint8_t* skip, int64_t* waitMs) {
    std::lock_guard<std::mutex> lk(mu_);
    return rl_retry_after(e_, n, key, permits, now, limiter, skip, waitMs);
}

int GpuEngine::quota(size_t n, const uint64_t* key, const int64_t* now, const uint16_t* limiter,
                     const int32_t* permits, const uint8_t* skip, int64_t* remaining, int64_t* resetMs,
                     int64_t* retryMs) {
    std::lock_guard<std::mutex> lk(mu_);
    return rl_quota(e_, n, key, now, limiter, permits, skip, remaining, resetMs, retryMs);
}

std::vector<std::pair<uint64_t, uint64_t>> GpuEngine::topKeys(const uint64_t* hashes, size_t n, uint32_t k,
                                                              uint64_t minCount) {
    if (k == 0 || k > RL_TOP_KEYS_MAX || minCount == 0 || (n && !hashes))
        throw IllegalArgumentException("topKeys: k in [1, RL_TOP_KEYS_MAX], minCount >= 1");
    std::vector<uint64_t> key(k), cnt(k);
    size_t nOut = 0;
    uint64_t nHeavy = 0;
    int st;
    {
        std::lock_guard<std::mutex> lk(mu_);
        st = rl_top_keys(e_, n, hashes, k, minCount, key.data(), cnt.data(), &nOut, &nHeavy);
    }
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("topKeys: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("topKeys: ") + rl_strerror(st), st);
    std::vector<std::pair<uint64_t, uint64_t>> out(nOut);
    for (size_t i = 0; i < nOut; ++i) out[i] = {key[i], cnt[i]};
    return out;
}

std::vector<std::pair<uint16_t, rl_limiter_tally>> GpuEngine::tallyBatch(size_t n, const int32_t* permits,
                                                                         const uint16_t* limiter,
                                                                         const uint8_t* op, const uint8_t* allowed,
                                                                         const int64_t* remaining) {
    std::vector<rl_limiter_tally> rows(RL_TALLY_ROWS);
    int st;
    {
        std::lock_guard<std::mutex> lk(mu_);
        st = rl_tally_batch(e_, n, permits, limiter, op, allowed, remaining, rows.data(), 0);
    }
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("tallyBatch: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("tallyBatch: ") + rl_strerror(st), st);
    std::vector<std::pair<uint16_t, rl_limiter_tally>> out;
    for (size_t r = 0; r < rows.size(); ++r)
        if (rows[r].requests) out.emplace_back((uint16_t)r, rows[r]);
    return out;
}

std::vector<std::pair<uint64_t, uint64_t>> GpuEngine::topDenied(size_t n, const uint64_t* hashes,
                                                                const int32_t* permits, const uint16_t* limiterIds,
                                                                const uint8_t* op, const uint8_t* allowed,
                                                                const int64_t* remaining, uint16_t limiter,
                                                                uint32_t k, uint64_t minCount, uint64_t* nDenied) {
    if (k == 0 || k > RL_TOP_KEYS_MAX || minCount == 0 || (n && !hashes))
        throw IllegalArgumentException("topDenied: k in [1, RL_TOP_KEYS_MAX], minCount >= 1");
    std::vector<uint64_t> key(k), cnt(k);
    size_t nOut = 0;
    uint64_t nHeavy = 0, denied = 0;
    int st;
    {
        std::lock_guard<std::mutex> lk(mu_);
        st = rl_top_denied(e_, n, hashes, permits, limiterIds, op, allowed, remaining, limiter, k, minCount,
                           key.data(), cnt.data(), &nOut, &nHeavy, &denied);
    }
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("topDenied: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("topDenied: ") + rl_strerror(st), st);
    if (nDenied) *nDenied = denied;
    std::vector<std::pair<uint64_t, uint64_t>> out(nOut);
    for (size_t i = 0; i < nOut; ++i) out[i] = {key[i], cnt[i]};
    return out;
}

rl_usage GpuEngine::usage(uint16_t limiter, int64_t nowNanos) {
    rl_usage u{};
    int st;
    {
        std::lock_guard<std::mutex> lk(mu_);
        st = rl_limiter_usage(e_, limiter, nowNanos, &u);
    }
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("usage: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("usage: ") + rl_strerror(st), st);
    return u;
}

std::vector<std::pair<uint64_t, int64_t>> GpuEngine::topConsumers(uint16_t limiter, int64_t nowNanos,
                                                                  uint32_t k, int64_t minUsed,
                                                                  uint64_t* nMatch) {
    if (k == 0 || k > RL_TOP_KEYS_MAX || minUsed < 0)
        throw IllegalArgumentException("topConsumers: k in [1, RL_TOP_KEYS_MAX], minUsed >= 0");
    std::vector<uint64_t> key(k);
    std::vector<int64_t> used(k);
    size_t nOut = 0;
    uint64_t matched = 0;
    int st;
    {
        std::lock_guard<std::mutex> lk(mu_);
        st = rl_top_consumers(e_, limiter, nowNanos, k, minUsed, key.data(), used.data(), &nOut, &matched);
    }
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("topConsumers: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("topConsumers: ") + rl_strerror(st), st);
    if (nMatch) *nMatch = matched;
    std::vector<std::pair<uint64_t, int64_t>> out(nOut);
    for (size_t i = 0; i < nOut; ++i) out[i] = {key[i], used[i]};
    return out;
}

size_t GpuEngine::snapshot(uint16_t limiter, size_t chunkImages, const SnapshotSink& sink) {
    const size_t cap = std::max<size_t>(chunkImages, RL_SNAPSHOT_MIN_CAP);
    std::vector<rl_key_image> buf(cap);
    std::lock_guard<std::mutex> lk(mu_);             // no batch of this object between the chunks
    size_t delivered = 0;
    uint64_t at = 0, total0 = 0;
    for (bool first = true;; first = false) {
        size_t n = 0;
        uint64_t done = 0, total = 0;
        const int st = rl_snapshot_keys(e_, limiter, at, ~0ULL, buf.data(), cap, &n, &done, &total);
        if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("snapshot: ") + rl_strerror(st));
        if (st != RL_OK) throw StorageException(std::string("snapshot: ") + rl_strerror(st), st);
        if (!first && total != total0)
            throw StorageException("snapshot: the table grew between two chunks", RL_E_INTERNAL);
        total0 = total;
        if (n && sink) sink(buf.data(), n);
        delivered += n;
        at += done;
        if (at >= total) return delivered;
    }
}

size_t GpuEngine::restore(const rl_key_image* images, size_t n) {
    if (n && !images) throw IllegalArgumentException("restore: null images");
    size_t put = 0;
    int st;
    {
        std::lock_guard<std::mutex> lk(mu_);
        st = rl_restore_keys(e_, n, images, &put);
    }
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("restore: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("restore: ") + rl_strerror(st), st);
    return put;
}

rl_shrink_report GpuEngine::shrink(uint16_t limiter, int64_t nowNanos, uint64_t minKeys) {
    rl_shrink_report r{};
    int st;
    {
        std::lock_guard<std::mutex> lk(mu_);
        st = rl_shrink_limiter(e_, limiter, nowNanos, minKeys, &r);
    }
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("shrink: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("shrink: ") + rl_strerror(st), st);
    return r;
}

rl_check_report GpuEngine::check(uint16_t limiter) {
    rl_check_report r{};
    int st;
    {
        std::lock_guard<std::mutex> lk(mu_);
        st = rl_check_limiter(e_, limiter, 0, ~0ULL, &r);
    }
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("check: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("check: ") + rl_strerror(st), st);
    return r;
}

rl_check_report GpuEngine::checkImages(const rl_key_image* images, size_t n) {
    if (n && !images) throw IllegalArgumentException("checkImages: null images");
    rl_check_report r{};
    int st;
    {
        std::lock_guard<std::mutex> lk(mu_);
        st = rl_check_images(e_, n, images, &r);
    }
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("checkImages: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("checkImages: ") + rl_strerror(st), st);
    return r;
}

// Throws unless the limiter exists and its table has at least bucketBits region bits (so nothing
// is sized by a bucketBits the engine would refuse); returns the table's region count.
static uint64_t digestRegions(rl_engine* e, uint16_t limiter, uint32_t bucketBits, const char* what) {
    uint64_t slots = 0;
    const int st = rl_limiter_slots(e, limiter, &slots);
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string(what) + ": " + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string(what) + ": " + rl_strerror(st), st);
    const uint64_t regions = slots / RL_SNAPSHOT_MIN_CAP;    // 256 slots each
    if (bucketBits > 63 || (regions >> bucketBits) == 0)
        throw IllegalArgumentException(std::string(what) + ": bucketBits beyond the table's region bits");
    return regions;
}

std::vector<rl_bucket_digest> GpuEngine::digest(uint16_t limiter, int64_t nowNanos, uint32_t bucketBits,
                                                bool withCache) {
    (void)digestRegions(e_, limiter, bucketBits, "digest");
    std::vector<rl_bucket_digest> out((size_t)1 << bucketBits);
    int st;
    {
        std::lock_guard<std::mutex> lk(mu_);
        st = rl_limiter_digest(e_, limiter, nowNanos, bucketBits, withCache ? RL_DIGEST_CACHE : 0u,
                               out.data(), nullptr);
    }
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("digest: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("digest: ") + rl_strerror(st), st);
    return out;
}

size_t GpuEngine::snapshotChanged(uint16_t limiter, int64_t nowNanos, uint32_t bucketBits,
                                  const std::vector<rl_bucket_digest>& previous,
                                  std::vector<rl_bucket_digest>* current, size_t chunkImages,
                                  const BucketSink& sink) {
    (void)digestRegions(e_, limiter, bucketBits, "snapshotChanged");
    if (!previous.empty() && previous.size() != (size_t)1 << bucketBits)
        throw IllegalArgumentException("snapshotChanged: previous must hold 2^bucketBits digests (or none)");
    const size_t nb = (size_t)1 << bucketBits;
    const size_t cap = std::max<size_t>(chunkImages, RL_SNAPSHOT_MIN_CAP);
    std::vector<rl_bucket_digest> now(nb);
    std::vector<rl_key_image> buf(cap);
    std::lock_guard<std::mutex> lk(mu_);             // no batch of this object between the calls
    int st = rl_limiter_digest(e_, limiter, nowNanos, bucketBits, RL_DIGEST_CACHE, now.data(), nullptr);
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string("snapshotChanged: ") + rl_strerror(st));
    if (st != RL_OK) throw StorageException(std::string("snapshotChanged: ") + rl_strerror(st), st);
    const uint64_t total0 = digestRegions(e_, limiter, bucketBits, "snapshotChanged");   // (held: as digested)
    const uint64_t per = total0 >> bucketBits;               // regions per bucket (>= 1: the digest was taken)
    size_t delivered = 0;
    for (size_t b = 0; b < nb; ++b) {
        if (!previous.empty() && previous[b].entries == now[b].entries && previous[b].sum == now[b].sum &&
            previous[b].xr == now[b].xr)
            continue;
        uint64_t at = b * per;
        const uint64_t end = at + per;
        bool called = false;
        while (at < end) {
            size_t n = 0;
            uint64_t done = 0, total = 0;
            st = rl_snapshot_keys(e_, limiter, at, end - at, buf.data(), cap, &n, &done, &total);
            if (st == RL_E_INVALID_ARG)
                throw IllegalArgumentException(std::string("snapshotChanged: ") + rl_strerror(st));
            if (st != RL_OK) throw StorageException(std::string("snapshotChanged: ") + rl_strerror(st), st);
            if (total != total0 || done == 0)
                throw StorageException("snapshotChanged: the table grew between two chunks", RL_E_INTERNAL);
            if (n && sink) { sink((uint32_t)b, buf.data(), n); called = true; }
            delivered += n;
            at += done;
        }
        if (!called && sink) sink((uint32_t)b, buf.data(), 0);
    }
    if (current) *current = std::move(now);
    return delivered;
}

GpuRateLimiter::GpuRateLimiter(std::shared_ptr<GpuEngine> engine, Algorithm algo,
                               const RateLimitConfig& cfg, Clock clock, int batchWindowMicros,
                               uint64_t smallBatch)
    : allowedRequests(algo == Algorithm::TokenBucket ? "ratelimiter.tokenbucket.allowed"
                                                      : "ratelimiter.requests.allowed"),
      rejectedRequests(algo == Algorithm::TokenBucket ? "ratelimiter.tokenbucket.rejected"
                                                       : "ratelimiter.requests.rejected"),
      engine_(std::move(engine)), algo_(algo), cfg_(cfg), clock_(std::move(clock)),
      windowMicros_(batchWindowMicros) {
    cfg_.validate();                                    // SlidingWindowRateLimiter.java:51
    if (algo == Algorithm::TokenBucket && !(cfg_.refillRate > 0))
        throw IllegalArgumentException(                // TokenBucketRateLimiter.java:77-79
            "Token bucket requires positive refillRate. Use RateLimitConfig.builder().refillRate(...)");
    id_ = engine_->addLimiter((int)algo, cfg_);
    if (smallBatch > 0) checkStatus(engine_->setSmallBatch(smallBatch), "setSmallBatch");
}

GpuRateLimiter::~GpuRateLimiter() { unpinFlush(); }

void GpuRateLimiter::unpinFlush() {
    if (fb_.cap == 0) return;
    engine_->unpin(fb_.key.data()); engine_->unpin(fb_.permits.data());
    engine_->unpin(fb_.now.data()); engine_->unpin(fb_.remaining.data());
    engine_->unpin(fb_.lim.data()); engine_->unpin(fb_.op.data()); engine_->unpin(fb_.allowed.data());
}

// Grow the flush buffers (doubling) and page-lock them once, so every later flush DMAs
// them directly (no pageable staging).
void GpuRateLimiter::reserveFlush(size_t n) {
    if (n <= fb_.cap) return;
    unpinFlush();
    size_t c = fb_.cap ? fb_.cap : 256;
    while (c < n) c *= 2;
    fb_.key.assign(c, 0); fb_.permits.assign(c, 0); fb_.now.assign(c, 0);
    fb_.remaining.assign(c, 0); fb_.lim.assign(c, id_); fb_.op.assign(c, 0); fb_.allowed.assign(c, 0);
    fb_.cap = c;
    engine_->pin(fb_.key.data(), c * 8); engine_->pin(fb_.permits.data(), c * 4);
    engine_->pin(fb_.now.data(), c * 8); engine_->pin(fb_.remaining.data(), c * 8);
    engine_->pin(fb_.lim.data(), c * 2); engine_->pin(fb_.op.data(), c);
    engine_->pin(fb_.allowed.data(), c);
}

void GpuRateLimiter::checkStatus(int st, const char* where) {
    if (st == RL_OK || st == RL_E_INVALID_REQUEST) return;
    if (st == RL_E_INVALID_ARG) throw IllegalArgumentException(std::string(where) + ": " + rl_strerror(st));
    throw StorageException(std::string(where) + ": " + rl_strerror(st), st);
}

// Leader-based micro-batcher: the first caller that finds no flush in progress waits
// `windowMicros_` for company, then runs every queued request as ONE engine batch in
// queue (arrival) order; the others sleep until their result is filled in.
// The request's clock is read here, under mu_, so queue order is clock order: two threads
// on one key can never enqueue their `now` values out of order (the engine's sliding
// window keeps a key's two newest buckets and assumes a key's time does not run
// backwards by more than a window).
void GpuRateLimiter::submit(Pending& p) {
    std::unique_lock<std::mutex> lk(mu_);
    p.now = clock_();
    queue_.push_back(&p);
    while (!p.done) {
        if (!flushing_) {
            flushing_ = true;
            if (windowMicros_ > 0) {
                lk.unlock();
                std::this_thread::sleep_for(std::chrono::microseconds(windowMicros_));
                lk.lock();
            }
            flushLocked(lk);
            flushing_ = false;
            cv_.notify_all();
        } else {
            cv_.wait(lk);
        }
    }
    if (p.status != RL_OK && p.status != RL_E_INVALID_REQUEST) checkStatus(p.status, "tryAcquire");
}

void GpuRateLimiter::flushLocked(std::unique_lock<std::mutex>& lk) {
    std::vector<Pending*> batch;
    batch.swap(queue_);
    lk.unlock();
    const size_t n = batch.size();
    reserveFlush(n);                    // the flush slot (flushing_) owns fb_
    uint64_t* k = fb_.key.data();
    int32_t* pm = fb_.permits.data();
    int64_t* t = fb_.now.data();
    uint8_t* op = fb_.op.data();
    for (size_t i = 0; i < n; ++i) {
        k[i] = batch[i]->key; pm[i] = batch[i]->permits; t[i] = batch[i]->now; op[i] = batch[i]->op;
    }
    uint64_t hits = 0;
    int st = engine_->executeBatch(n, k, pm, t, fb_.lim.data(), op, fb_.allowed.data(),
                                   fb_.remaining.data(), &hits);
    const uint8_t* al = fb_.allowed.data();
    const int64_t* rem = fb_.remaining.data();
    cacheHits.increment(hits);
    lk.lock();
    for (size_t i = 0; i < n; ++i) {
        batch[i]->allowed = al[i];
        batch[i]->remaining = rem[i];
        batch[i]->status = st;
        batch[i]->done = true;
    }
}

void GpuRateLimiter::requirePositive(int permits) {
    if (permits <= 0) throw IllegalArgumentException("permits must be positive");  // :87-89 / :106-108
}

bool GpuRateLimiter::tryAcquire(const std::string& key, int permits) {
    requirePositive(permits);
    Pending p{keyHash(key), permits, 0, RL_OP_ACQUIRE};
    submit(p);
    if (p.allowed) allowedRequests.increment();
    else rejectedRequests.increment();
    return p.allowed != 0;
}

int64_t GpuRateLimiter::getAvailablePermits(const std::string& key) {
    Pending p{keyHash(key), 1, 0, RL_OP_PEEK};
    submit(p);
    return p.remaining;
}

void GpuRateLimiter::reset(const std::string& key) {
    Pending p{keyHash(key), 1, 0, RL_OP_RESET};
    submit(p);
}

int64_t GpuRateLimiter::retryAfterMillis(const std::string& key, int permits) {
    requirePositive(permits);
    const uint64_t k = keyHash(key);
    const int32_t p = permits;
    int64_t now = 0, wait = 0;
    int st;
    {
        // behind every tryAcquire that has returned: wait out a flush in progress and hold
        // the flush slot while the query runs (as tryAcquireBatch does); the clock is read
        // under mu_, like a request's
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !flushing_; });
        flushing_ = true;
        now = clock_();
        lk.unlock();
        st = engine_->retryAfter(1, &k, &p, &now, &id_, nullptr, &wait);
        lk.lock();
        flushing_ = false;
        cv_.notify_all();
    }
    checkStatus(st, "retryAfterMillis");
    if (st == RL_E_INVALID_REQUEST || wait == RL_RETRY_INVALID)
        throw IllegalArgumentException("retryAfterMillis: invalid request");
    return wait;                                     // RL_RETRY_NEVER = -1: never
}

RateLimitQuota GpuRateLimiter::quota(const std::string& key, int permits) {
    requirePositive(permits);
    const uint64_t k = keyHash(key);
    const int32_t p = permits;
    int64_t now = 0;
    RateLimitQuota q{cfg_.maxPermits, 0, 0, 0};
    int st;
    {
        // ordered and clocked as retryAfterMillis is
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !flushing_; });
        flushing_ = true;
        now = clock_();
        lk.unlock();
        st = engine_->quota(1, &k, &now, &id_, &p, nullptr, &q.remaining, &q.resetMillis,
                            &q.retryAfterMillis);
        lk.lock();
        flushing_ = false;
        cv_.notify_all();
    }
    checkStatus(st, "quota");
    if (st == RL_E_INVALID_REQUEST || q.resetMillis == RL_QUOTA_INVALID)
        throw IllegalArgumentException("quota: invalid request");
    return q;                                        // retryAfterMillis RL_RETRY_NEVER = -1: never
}

// The census calls run like retryAfterMillis: behind every tryAcquire that has returned, holding
// the flush slot, with the clock read under mu_.
rl_usage GpuRateLimiter::usage() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return !flushing_; });
    flushing_ = true;
    const int64_t now = clock_();
    lk.unlock();
    struct Release {
        GpuRateLimiter* self; std::unique_lock<std::mutex>& lk;
        ~Release() { lk.lock(); self->flushing_ = false; self->cv_.notify_all(); }
    } rel{this, lk};
    return engine_->usage(id_, now);
}

std::vector<rl_bucket_digest> GpuRateLimiter::digest(uint32_t bucketBits) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return !flushing_; });
    flushing_ = true;
    const int64_t now = clock_();
    lk.unlock();
    struct Release {
        GpuRateLimiter* self; std::unique_lock<std::mutex>& lk;
        ~Release() { lk.lock(); self->flushing_ = false; self->cv_.notify_all(); }
    } rel{this, lk};
    return engine_->digest(id_, now, bucketBits);
}

rl_check_report GpuRateLimiter::check() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return !flushing_; });
    flushing_ = true;
    lk.unlock();
    struct Release {
        GpuRateLimiter* self; std::unique_lock<std::mutex>& lk;
        ~Release() { lk.lock(); self->flushing_ = false; self->cv_.notify_all(); }
    } rel{this, lk};
    return engine_->check(id_);
}

rl_shrink_report GpuRateLimiter::compact() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return !flushing_; });
    flushing_ = true;
    const int64_t now = clock_();
    lk.unlock();
    struct Release {
        GpuRateLimiter* self; std::unique_lock<std::mutex>& lk;
        ~Release() { lk.lock(); self->flushing_ = false; self->cv_.notify_all(); }
    } rel{this, lk};
    return engine_->shrink(id_, now, cfg_.expectedKeys);
}

std::vector<std::pair<uint64_t, int64_t>> GpuRateLimiter::topConsumers(uint32_t k, int64_t minUsed) {
    if (k == 0 || k > RL_TOP_KEYS_MAX || minUsed < 0)
        throw IllegalArgumentException("topConsumers: k in [1, RL_TOP_KEYS_MAX], minUsed >= 0");
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return !flushing_; });
    flushing_ = true;
    const int64_t now = clock_();
    lk.unlock();
    struct Release {
        GpuRateLimiter* self; std::unique_lock<std::mutex>& lk;
        ~Release() { lk.lock(); self->flushing_ = false; self->cv_.notify_all(); }
    } rel{this, lk};
    return engine_->topConsumers(id_, now, k, minUsed);
}

void GpuRateLimiter::acquireBatch(size_t n, const BatchCall& run, bool* allowed, int64_t* remaining) {
    if (n == 0) return;
    std::vector<uint16_t> lim(n, id_);
    std::vector<uint8_t> al(n);
    std::vector<int64_t> rem(n);
    int st;
    {
        // keep arrival order with single calls: wait out a flush in progress (it runs with
        // mu_ released) and hold the flush slot while this batch runs
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !flushing_; });
        flushing_ = true;
        lk.unlock();
        uint64_t hits = 0;
        st = run(lim.data(), al.data(), rem.data(), &hits);
        cacheHits.increment(hits);
        lk.lock();
        flushing_ = false;
        cv_.notify_all();
    }
    checkStatus(st, "tryAcquireBatch");
    uint64_t ok = 0;
    for (size_t i = 0; i < n; ++i) {
        allowed[i] = al[i] != 0;
        ok += al[i];
        if (remaining) remaining[i] = rem[i];
    }
    allowedRequests.increment(ok);
    rejectedRequests.increment(n - ok);
}

void GpuRateLimiter::tryAcquireBatch(size_t n, const uint64_t* keyHash, const int32_t* permits,
                                     const int64_t* nowNanos, bool* allowed, int64_t* remaining) {
    acquireBatch(n, [&](const uint16_t* lim, uint8_t* al, int64_t* rem, uint64_t* hits) {
        return engine_->executeBatch(n, keyHash, permits, nowNanos, lim, nullptr, al, rem, hits);
    }, allowed, remaining);
}

void GpuRateLimiter::tryAcquireBatch(const KeyBatch& keys, const int32_t* permits, const int64_t* nowNanos,
                                     bool* allowed, int64_t* remaining, uint64_t* keyHashOut) {
    acquireBatch(keys.size(), [&](const uint16_t* lim, uint8_t* al, int64_t* rem, uint64_t* hits) {
        return engine_->executeBatchKeys(keys, permits, nowNanos, lim, nullptr, al, rem, keyHashOut, hits);
    }, allowed, remaining);
}

}  // namespace ratelimiter
