// Tests of the small-batch option of the C++ mirror (distributed-rate-limiter_amd/host).
//   test_small_host cpu : argument checks of rl_small_batches (no device calls)
//   test_small_host gpu : two engines with the same two limiters on string keys and a pinned
//                         clock (a sliding window with the local cache, a token bucket), one
//                         with GpuRateLimiter's smallBatch option on and one with it off, take
//                         the same single tryAcquire / getAvailablePermits / reset calls over
//                         several windows. Every call answers the same on both, the first
//                         engine's smallBatches().taken counts every one of them and the
//                         second's stays 0.
#include <cstdio>
#include <memory>
#include <string>

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

static void cpu_tests() {
    uint64_t taken = 7, declined = 9;
    CHECK(rl_small_batches(nullptr, &taken, &declined) == RL_E_INVALID_ARG);
    CHECK(taken == 7 && declined == 9);
    CHECK(rl_small_batches(nullptr, nullptr, nullptr) == RL_E_INVALID_ARG);
    CHECK(rl_tune(nullptr, "small_batch", 1) == RL_E_INVALID_ARG);
    CHECK(RL_SMALL_BATCH_MAX >= 1024);
}

static void gpu_tests() {
    GpuEngine::Options o;
    o.maxBatch = 1 << 12;
    o.defaultCapacity = 1 << 10;
    auto ea = std::make_shared<GpuEngine>(o), eb = std::make_shared<GpuEngine>(o);
    RateLimitConfig sc;
    sc.maxPermits = 3;
    sc.windowMs = 1000;
    sc.localCacheTtlMs = 300;                                    // (enableLocalCache defaults to true)
    RateLimitConfig tc;
    tc.maxPermits = 5;
    tc.windowMs = 1000;
    tc.refillRate = 2.0;
    int64_t t_ms = 1700000000000LL + 100;
    const Clock clock = [&] { return t_ms * 1000000; };
    GpuRateLimiter swA(ea, GpuRateLimiter::Algorithm::SlidingWindow, sc, clock, 0, 64);
    GpuRateLimiter tbA(ea, GpuRateLimiter::Algorithm::TokenBucket, tc, clock, 0, 64);
    GpuRateLimiter swB(eb, GpuRateLimiter::Algorithm::SlidingWindow, sc, clock, 0, 0);
    GpuRateLimiter tbB(eb, GpuRateLimiter::Algorithm::TokenBucket, tc, clock, 0, 0);
    CHECK(ea->smallBatches().first == 0 && ea->smallBatches().second == 0);

    uint64_t calls = 0;
    int allowed = 0, denied = 0;
    for (int round = 0; round < 6; ++round) {
        for (int i = 0; i < 12; ++i) {
            const std::string user = "user-" + std::to_string(i % 5);
            const bool a = swA.tryAcquire(user), b = swB.tryAcquire(user);
            CHECK(a == b);
            (a ? allowed : denied) += 1;
            CHECK(tbA.tryAcquire(user, 1 + i % 3) == tbB.tryAcquire(user, 1 + i % 3));
            CHECK(swA.getAvailablePermits(user) == swB.getAvailablePermits(user));
            CHECK(tbA.getAvailablePermits(user) == tbB.getAvailablePermits(user));
            calls += 4;                                          // engine A's: two acquires, two peeks
            if (i == 7) {
                swA.reset(user); swB.reset(user);
                tbA.reset(user); tbB.reset(user);
                calls += 2;                                      // (engine A's two)
            }
            t_ms += 23;
        }
        t_ms += round % 2 ? 900 : 150;                           // inside the window and the cache TTL, past both
    }
    CHECK(allowed > 0 && denied > 0);
    CHECK(swA.allowedRequests.count() == swB.allowedRequests.count());
    CHECK(swA.rejectedRequests.count() == swB.rejectedRequests.count());
    CHECK(swA.cacheHits.count() == swB.cacheHits.count() && swA.cacheHits.count() > 0);
    CHECK(tbA.allowedRequests.count() == tbB.allowedRequests.count());
    const auto ta = ea->smallBatches(), tb = eb->smallBatches();
    CHECK(ta.first == calls && ta.second == 0);
    CHECK(tb.first == 0 && tb.second == 0);
    // the option off again: the same engine goes on through the pipeline
    CHECK(ea->setSmallBatch(0) == RL_OK);
    CHECK(swA.tryAcquire("user-1") == swB.tryAcquire("user-1"));
    CHECK(ea->smallBatches().first == calls);
    CHECK(ea->setSmallBatch(1) == RL_OK);
    CHECK(swA.tryAcquire("user-2") == swB.tryAcquire("user-2"));
    CHECK(ea->smallBatches().first == calls + 1);
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "cpu") cpu_tests();
    else if (mode == "gpu") gpu_tests();
    else { std::fprintf(stderr, "usage: test_small_host cpu|gpu\n"); return 2; }
    if (failures) { std::printf("%s: %d FAILED\n", mode.c_str(), failures); return 1; }
    std::printf("%s: ok\n", mode.c_str());
    return 0;
}
