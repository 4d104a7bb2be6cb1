// Tests of GpuRateLimiter::usage / topConsumers (distributed-rate-limiter_amd/host).
//   test_usage cpu : argument checks of the C calls and of the mirror's own (no device calls)
//   test_usage gpu : a sliding window (3 per minute) on string keys with a pinned clock: user i
//                    tries i times, so used = min(i, 3); the census and the heaviest consumers
//                    against keyHash() of the strings
#include <algorithm>
#include <cstdio>
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
    CHECK(RL_USAGE_BINS == 16 && RL_USAGE_CANDIDATES == 65536);
    CHECK(sizeof(rl_usage) == 8 * (7 + 16));
    rl_usage u;
    u.live_keys = 7;
    uint64_t key[2] = {7, 7}, n_match = 7;
    int64_t used[2] = {7, 7};
    size_t n_out = 7;
    CHECK(rl_limiter_usage(nullptr, 0, 0, &u) == RL_E_INVALID_ARG);
    CHECK(rl_top_consumers(nullptr, 0, 0, 2, 1, key, used, &n_out, &n_match) == RL_E_INVALID_ARG);
    CHECK(u.live_keys == 7 && key[0] == 7 && used[1] == 7 && n_out == 7 && n_match == 7);
}

using Pairs = std::vector<std::pair<uint64_t, int64_t>>;

static void gpu_tests() {
    GpuEngine::Options o;
    o.maxBatch = 1 << 12;
    o.defaultCapacity = 1 << 10;
    auto eng = std::make_shared<GpuEngine>(o);
    RateLimitConfig c;
    c.maxPermits = 3;
    c.windowMs = 60000;
    c.enableLocalCache = false;
    int64_t t_ms = 1700000000000LL / 60000 * 60000 + 30000;      // mid-window
    GpuRateLimiter sw(eng, GpuRateLimiter::Algorithm::SlidingWindow, c,
                      [&] { return t_ms * 1000000; });
    // bad arguments throw before anything reaches the engine
    CHECK(throws<IllegalArgumentException>([&] { sw.topConsumers(0, 1); }));
    CHECK(throws<IllegalArgumentException>([&] { sw.topConsumers(RL_TOP_KEYS_MAX + 1, 1); }));
    CHECK(throws<IllegalArgumentException>([&] { sw.topConsumers(4, -1); }));
    CHECK(throws<IllegalArgumentException>([&] { eng->usage(200, 0); }));   // unknown limiter
    // an empty limiter
    rl_usage u = sw.usage();
    CHECK(u.slots > 0 && u.used_slots == 0 && u.live_keys == 0 && u.redis_keys == 0 && u.used_permits == 0);
    CHECK(sw.topConsumers(4, 0).empty());

    Pairs want;                                   // (hash, used) of every user with a request
    uint64_t allowed = 0;
    for (int i = 0; i < 10; ++i) {
        const std::string user = "user-" + std::to_string(i);
        for (int j = 0; j < i; ++j) allowed += sw.tryAcquire(user) ? 1 : 0;
        if (i) want.push_back({keyHash(user), std::min(i, 3)});
        t_ms += 7;
    }
    CHECK(allowed == 1 + 2 + 3 * 7);
    std::sort(want.begin(), want.end(), [](const auto& a, const auto& b) {
        return a.second != b.second ? a.second > b.second : a.first < b.first;
    });
    u = sw.usage();
    CHECK(u.live_keys == 9 && u.redis_keys == 9 && u.used_slots == 9);
    CHECK(u.exhausted_keys == 7 && u.cache_blocked == 0 && u.used_permits == 24);
    uint64_t sum = 0;
    for (uint64_t h : u.hist) sum += h;
    CHECK(sum == 9 && u.hist[15] == 7 && u.hist[10] == 1 && u.hist[5] == 1);   // used * 16 / 3
    uint64_t slots = 0;
    CHECK(rl_limiter_slots(eng->handle(), sw.limiterId(), &slots) == RL_OK && slots == u.slots);

    CHECK(sw.topConsumers(4096, 1) == want);
    CHECK(sw.topConsumers(4096, 0) == want);
    CHECK(sw.topConsumers(4) == Pairs(want.begin(), want.begin() + 4));      // inside the tie at 3
    CHECK(sw.topConsumers(8, 3) == Pairs(want.begin(), want.begin() + 7));
    uint64_t n_match = 0;
    CHECK(eng->topConsumers(sw.limiterId(), t_ms * 1000000, 2, 2, &n_match).size() == 2 && n_match == 8);
    // read-only: the throttled keys stay throttled, the others keep their room
    CHECK(!sw.tryAcquire("user-9") && sw.getAvailablePermits("user-1") == 2);
    // a window and a half later nothing is live
    t_ms += 2 * 60000;
    u = sw.usage();
    CHECK(u.live_keys == 0 && u.exhausted_keys == 0 && u.used_slots >= 9);   // tombstones stay
    CHECK(sw.topConsumers(4, 0).empty());
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    cpu_tests();
    if (mode == "gpu") gpu_tests();
    std::printf("%s: %s (%d failures)\n", mode.c_str(), failures ? "FAIL" : "ok", failures);
    return failures ? 1 : 0;
}
