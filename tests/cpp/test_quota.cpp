// Tests of GpuRateLimiter::quota / GpuEngine::quota (distributed-rate-limiter_amd/host).
//   test_quota cpu  : argument mapping, constants, the C calls' checks (no device calls)
//   test_quota gpu  : a token bucket (5 @ 10/s) and a sliding window after a few acquires, under
//                     a clock the test owns: quota() against getAvailablePermits and
//                     retryAfterMillis at the same instant
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

template <class E, class F>
static bool throws(F f) {
    try { f(); } catch (const E&) { return true; } catch (...) { return false; }
    return false;
}

static void cpu_tests() {
    CHECK(RL_QUOTA_INVALID == -2);
    // the struct's fields in header order: limit, remaining, reset, retry-after
    const RateLimitQuota q{10, 7, 130, -1};
    CHECK(q.limit == 10 && q.remaining == 7 && q.resetMillis == 130 && q.retryAfterMillis == -1);
    // permits <= 0 never reaches the engine (quota() checks as tryAcquire does)
    CHECK(throws<IllegalArgumentException>([] { GpuRateLimiter::requirePositive(0); }));
    // the C calls reject a null engine before any device call, whatever else is passed
    uint64_t k = 1;
    int32_t p = 1;
    uint8_t sk = 0;
    int64_t now = 0, rem = 7, reset = 7, retry = 7;
    CHECK(rl_quota(nullptr, 1, &k, &now, nullptr, &p, nullptr, &rem, &reset, &retry) == RL_E_INVALID_ARG);
    CHECK(rl_quota(nullptr, 1, &k, &now, nullptr, nullptr, nullptr, &rem, &reset, nullptr) == RL_E_INVALID_ARG);
    CHECK(rl_quota(nullptr, 1, &k, &now, nullptr, &p, nullptr, &rem, &reset, nullptr) == RL_E_INVALID_ARG);
    CHECK(rl_quota(nullptr, 1, &k, &now, nullptr, nullptr, &sk, &rem, &reset, nullptr) == RL_E_INVALID_ARG);
    CHECK(rl_quota(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
          RL_E_INVALID_ARG);
    CHECK(rl_quota_device(nullptr, 1, &k, &now, nullptr, &p, nullptr, &rem, &reset, &retry, nullptr) ==
          RL_E_INVALID_ARG);
    CHECK(rem == 7 && reset == 7 && retry == 7);
}

static void gpu_tests() {
    auto eng = std::make_shared<GpuEngine>();
    int64_t ms = 1700000000000LL;                         // the test's clock
    Clock clock = [&ms] { return ms * 1000000LL; };

    RateLimitConfig c;
    c.maxPermits = 5;
    c.windowMs = 1000;
    c.refillRate = 10.0;                                  // one token per 100 ms
    GpuRateLimiter tb(eng, GpuRateLimiter::Algorithm::TokenBucket, c, clock);
    CHECK(throws<IllegalArgumentException>([&] { tb.quota("k", 0); }));
    CHECK(throws<IllegalArgumentException>([&] { tb.quota("k", -1); }));
    RateLimitQuota q = tb.quota("absent");
    CHECK(q.limit == 5 && q.remaining == 5 && q.resetMillis == 0 && q.retryAfterMillis == 0);

    CHECK(tb.tryAcquire("user", 3));                      // 2 left at ms
    ms += 50;                                             // 2.5 tokens
    q = tb.quota("user", 3);
    CHECK(q.limit == 5);
    CHECK(q.remaining == 2 && q.remaining == tb.getAvailablePermits("user"));
    CHECK(q.retryAfterMillis == 50 && q.retryAfterMillis == tb.retryAfterMillis("user", 3));
    CHECK(q.resetMillis == 250 && q.resetMillis == tb.retryAfterMillis("user", 5));
    CHECK(tb.quota("user", 6).retryAfterMillis == -1);    // permits > maxPermits: never
    CHECK(tb.quota("user", 6).resetMillis == 250);
    CHECK(tb.quota("user").retryAfterMillis == 0);        // default permits = 1
    ms += 249;
    CHECK(tb.quota("user").resetMillis == 1 && tb.getAvailablePermits("user") == 4);
    ms += 1;
    q = tb.quota("user");
    CHECK(q.resetMillis == 0 && q.remaining == 5 && tb.getAvailablePermits("user") == 5);
    // read-only: the queries above took nothing
    CHECK(tb.allowedRequests.count() == 1 && tb.rejectedRequests.count() == 0);

    RateLimitConfig s;
    s.maxPermits = 3;
    s.windowMs = 1000;
    s.enableLocalCache = false;                           // so that reset == retry-after of maxPermits
    GpuRateLimiter sw(eng, GpuRateLimiter::Algorithm::SlidingWindow, s, clock);
    ms = 1700000010000LL;                                 // a window start
    CHECK(sw.tryAcquire("user") && sw.tryAcquire("user"));
    ms += 400;
    CHECK(sw.tryAcquire("user"));                         // 3 in this window, the last at +400
    CHECK(!sw.tryAcquire("user"));
    ms += 100;
    q = sw.quota("user", 1);
    CHECK(q.limit == 3 && q.remaining == 0 && q.remaining == sw.getAvailablePermits("user"));
    CHECK(q.retryAfterMillis == sw.retryAfterMillis("user", 1));
    // one permit is back once 3 * (1 - f) + 0 < 3 reads 2: in the next window, f > 0
    CHECK(q.retryAfterMillis == 501);
    // the full quota is back when the bucket's PEXPIRE (last INCR + w) lapses: +400 + 1000 + 1
    CHECK(q.resetMillis == 901 && q.resetMillis == sw.retryAfterMillis("user", 3));
    ms += 900;
    CHECK(sw.getAvailablePermits("user") < 3 && sw.quota("user").resetMillis == 1);
    ms += 1;
    CHECK(sw.getAvailablePermits("user") == 3 && sw.quota("user").resetMillis == 0);
    sw.reset("user");
    CHECK(sw.quota("user").remaining == 3);
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    cpu_tests();
    if (mode == "gpu") gpu_tests();
    std::printf("%s: %s (%d failures)\n", mode.c_str(), failures ? "FAIL" : "ok", failures);
    return failures ? 1 : 0;
}
