// Tests of GpuEngine::snapshot / restore (distributed-rate-limiter_amd/host).
//   test_snapshot cpu : argument checks of the four C calls (no device calls)
//   test_snapshot gpu : two limiters on string keys with a pinned clock (a sliding window with the
//                       local cache, a token bucket) build state on engine A; A is snapshotted in
//                       chunks of one region's worth of images and restored into a fresh engine B;
//                       every later tryAcquire / getAvailablePermits then answers the same on both
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../distributed-rate-limiter_amd/host/ratelimiter.hpp"

using namespace ratelimiter;

static int failures = 0;
#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                            \
        }                                                                          \
    } while (0)

template <class E, class F>
static bool throws(F f) {
    try { f(); } catch (const E&) { return true; } catch (...) { return false; }
    return false;
}

static void cpu_tests() {
    CHECK(RL_SNAPSHOT_MIN_CAP == 256 && sizeof(rl_key_image) == 48);
    std::vector<rl_key_image> img(4);
    std::memset(img.data(), 0x5A, img.size() * sizeof(rl_key_image));
    const std::vector<rl_key_image> before = img;
    size_t n = 7;
    uint64_t done = 7, total = 7, hdr[4] = {7, 7, 7, 7};
    CHECK(rl_snapshot_keys(nullptr, 0, 0, 1, img.data(), 4, &n, &done, &total) == RL_E_INVALID_ARG);
    CHECK(rl_snapshot_keys_device(nullptr, 0, 0, 1, img.data(), 4, hdr, nullptr) == RL_E_INVALID_ARG);
    CHECK(rl_put_keys_device(nullptr, 4, img.data(), hdr, nullptr) == RL_E_INVALID_ARG);
    CHECK(rl_restore_keys(nullptr, 4, img.data(), &n) == RL_E_INVALID_ARG);
    CHECK(n == 7 && done == 7 && total == 7 && hdr[0] == 7 && hdr[3] == 7);
    CHECK(std::memcmp(img.data(), before.data(), img.size() * sizeof(rl_key_image)) == 0);
}

using Images = std::vector<rl_key_image>;

static Images snapshot_of(GpuEngine& e, uint16_t limiter, size_t chunk, size_t* chunks) {
    Images all;
    *chunks = 0;
    const size_t n = e.snapshot(limiter, chunk, [&](const rl_key_image* im, size_t k) {
        all.insert(all.end(), im, im + k);
        ++*chunks;
    });
    CHECK(n == all.size());
    return all;
}

static Images sorted(Images v) {
    std::sort(v.begin(), v.end(), [](const rl_key_image& a, const rl_key_image& b) {
        return a.limiter != b.limiter ? a.limiter < b.limiter : a.key_hash < b.key_hash;
    });
    return v;
}

static bool same(const Images& a, const Images& b) {
    return a.size() == b.size() &&
           (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(rl_key_image)) == 0);
}

static void gpu_tests() {
    GpuEngine::Options o;
    o.maxBatch = 1 << 12;
    o.defaultCapacity = 1 << 10;
    auto ea = std::make_shared<GpuEngine>(o), eb = std::make_shared<GpuEngine>(o);
    RateLimitConfig sc;
    sc.maxPermits = 3;
    sc.windowMs = 60000;
    sc.localCacheTtlMs = 5000;                                   // (enableLocalCache defaults to true)
    RateLimitConfig tc;
    tc.maxPermits = 5;
    tc.windowMs = 60000;
    tc.refillRate = 0.3;
    int64_t t_ms = 1700000000000LL / 60000 * 60000 + 30000;      // mid-window
    const Clock clock = [&] { return t_ms * 1000000; };
    GpuRateLimiter swA(ea, GpuRateLimiter::Algorithm::SlidingWindow, sc, clock);
    GpuRateLimiter tbA(ea, GpuRateLimiter::Algorithm::TokenBucket, tc, clock);
    GpuRateLimiter swB(eb, GpuRateLimiter::Algorithm::SlidingWindow, sc, clock);
    GpuRateLimiter tbB(eb, GpuRateLimiter::Algorithm::TokenBucket, tc, clock);
    CHECK(swA.limiterId() == swB.limiterId() && tbA.limiterId() == tbB.limiterId());
    CHECK(throws<IllegalArgumentException>([&] { ea->snapshot(200, 256, nullptr); }));   // unknown limiter

    // an empty table: no chunk, no image
    size_t chunks = 7;
    CHECK(snapshot_of(*ea, swA.limiterId(), 256, &chunks).empty() && chunks == 0);

    // user i tries i % 5 times under the window (the fourth try is denied and, with the third
    // allow, leaves a cache entry) and takes i % 7 tokens from its bucket
    const int kUsers = 400;
    for (int i = 0; i < kUsers; ++i) {
        const std::string user = "user-" + std::to_string(i);
        for (int j = 0; j < i % 5; ++j) (void)swA.tryAcquire(user);
        if (i % 7) (void)tbA.tryAcquire(user, std::min(i % 7, 5));
        t_ms += 3;
    }
    swA.reset("user-9");                                         // a tombstone: no image
    t_ms += 50;

    const rl_usage ua = swA.usage();
    Images all;
    for (uint16_t lim : {swA.limiterId(), tbA.limiterId()}) {
        const Images part = snapshot_of(*ea, lim, 256, &chunks);
        CHECK(chunks >= 2);                                      // > 256 images: several chunks
        for (const rl_key_image& im : part) CHECK(im.limiter == lim);
        all.insert(all.end(), part.begin(), part.end());
    }
    CHECK(all.size() == (size_t)(kUsers - kUsers / 5 - 1) + (size_t)(kUsers - (kUsers + 6) / 7));
    CHECK(same(sorted(snapshot_of(*ea, swA.limiterId(), 1 << 16, &chunks)),
               sorted(Images(all.begin(), all.begin() + (kUsers - kUsers / 5 - 1)))) && chunks == 1);
    const rl_usage ua2 = swA.usage();
    CHECK(std::memcmp(&ua, &ua2, sizeof(ua)) == 0);              // read-only

    CHECK(eb->restore(all.data(), all.size()) == all.size());
    Images allB;
    for (uint16_t lim : {swB.limiterId(), tbB.limiterId()}) {
        const Images part = snapshot_of(*eb, lim, 4096, &chunks);
        allB.insert(allB.end(), part.begin(), part.end());
    }
    CHECK(same(sorted(all), sorted(allB)));
    const rl_usage ub = swB.usage();
    CHECK(ub.live_keys == ua.live_keys && ub.used_permits == ua.used_permits &&
          ub.cache_blocked == ua.cache_blocked && ub.exhausted_keys == ua.exhausted_keys);
    CHECK(ua.cache_blocked > 0);

    // the clone decides as the original: inside the cache TTL, after it, and a window later
    int denied = 0, allowed = 0;
    for (int round = 0; round < 3; ++round) {
        for (int i = 0; i < kUsers; i += (round ? 3 : 1)) {
            const std::string user = "user-" + std::to_string(i);
            CHECK(swA.getAvailablePermits(user) == swB.getAvailablePermits(user));
            const bool a = swA.tryAcquire(user), b = swB.tryAcquire(user);
            CHECK(a == b);
            (a ? allowed : denied) += 1;
            CHECK(tbA.tryAcquire(user, 2) == tbB.tryAcquire(user, 2));
            CHECK(tbA.getAvailablePermits(user) == tbB.getAvailablePermits(user));
        }
        t_ms += round ? 40000 : 6000;
    }
    CHECK(denied > 50 && allowed > 50);
    CHECK(same(sorted(snapshot_of(*ea, swA.limiterId(), 4096, &chunks)),
               sorted(snapshot_of(*eb, swB.limiterId(), 4096, &chunks))));
    // unordered images take the fallback and give the same table
    auto ec = std::make_shared<GpuEngine>(o);
    GpuRateLimiter swC(ec, GpuRateLimiter::Algorithm::SlidingWindow, sc, clock);
    GpuRateLimiter tbC(ec, GpuRateLimiter::Algorithm::TokenBucket, tc, clock);
    Images rev(all.rbegin(), all.rend());
    CHECK(ec->restore(rev.data(), rev.size()) == rev.size());
    Images allC;
    for (uint16_t lim : {swC.limiterId(), tbC.limiterId()}) {
        const Images part = snapshot_of(*ec, lim, 4096, &chunks);
        allC.insert(allC.end(), part.begin(), part.end());
    }
    CHECK(same(sorted(all), sorted(allC)));
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    cpu_tests();
    if (mode == "gpu") gpu_tests();
    std::printf("%s: %s (%d failures)\n", mode.c_str(), failures ? "FAIL" : "ok", failures);
    return failures ? 1 : 0;
}
