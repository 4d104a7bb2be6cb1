// Tests of GpuEngine::digest / snapshotChanged and GpuRateLimiter::digest
// (distributed-rate-limiter_amd/host).
//   test_digest cpu : argument checks of the C calls, the structure and the constants (no device
//                     calls)
//   test_digest gpu : a sliding window with its local cache and a token bucket on 3000 string
//                     keys with a pinned clock. The digests against a restatement of the header's
//                     definition over rl_export_state output; a per-bucket checkpoint built with
//                     snapshotChanged, brought up to date after traffic that touches known
//                     buckets (one of them emptied by resets), restored into a fresh engine of
//                     another size: same digests, same decisions on one further batch.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <set>
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

// ---- the header's definition, restated
static uint64_t mix(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27; x *= 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}
static uint64_t rotl(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
static uint64_t entryHash(uint64_t keyHash, uint64_t k, uint64_t f1, uint64_t f2, uint64_t f3) {
    uint64_t u = mix(keyHash) + k;
    u = (u ^ f1) * RL_DIGEST_C1;
    u = (u ^ rotl(f2, 23)) * RL_DIGEST_C2;
    u ^= rotl(f3, 47);
    return mix(u);
}
static uint32_t bucketOf(uint64_t keyHash, uint32_t bits) {
    return bits ? (uint32_t)(mix(keyHash) >> (64 - bits)) : 0;
}

static bool same(const rl_bucket_digest& a, const rl_bucket_digest& b) {
    return a.entries == b.entries && a.sum == b.sum && a.xr == b.xr;
}
static bool same(const std::vector<rl_bucket_digest>& a, const std::vector<rl_bucket_digest>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!same(a[i], b[i])) return false;
    return true;
}

// The digests (no cache entries) of one limiter from the engine's Redis-layout export.
static std::vector<rl_bucket_digest> fromExport(rl_engine* e, uint16_t limiter, int64_t nowNanos, uint32_t bits) {
    std::vector<rl_state_entry> ent(1 << 16);
    size_t n = 0;
    CHECK(rl_export_state(e, nowNanos, ent.data(), ent.size(), &n) == RL_OK);
    std::vector<rl_bucket_digest> out((size_t)1 << bits, rl_bucket_digest{0, 0, 0});
    for (size_t i = 0; i < n; ++i) {
        const rl_state_entry& s = ent[i];
        if (s.limiter != limiter) continue;
        uint64_t h;
        if (s.kind == RL_STATE_TB_BUCKET) {
            uint64_t tok;
            std::memcpy(&tok, &s.tokens, 8);
            h = entryHash(s.key_hash, RL_DIGEST_K_TB, tok, (uint64_t)s.last_refill_ms, (uint64_t)s.expire_at_ms);
        } else {
            h = entryHash(s.key_hash, RL_DIGEST_K_SW, (uint64_t)s.window_start_ms, (uint64_t)s.count,
                          (uint64_t)s.expire_at_ms);
        }
        rl_bucket_digest& d = out[bucketOf(s.key_hash, bits)];
        d.entries += 1; d.sum += h; d.xr ^= h;
    }
    return out;
}

static void cpu_tests() {
    CHECK(sizeof(rl_bucket_digest) == 24 && RL_DIGEST_CACHE == 1u && RL_ABI_VERSION == 3);
    for (uint64_t c : {RL_DIGEST_K_SW, RL_DIGEST_K_TB, RL_DIGEST_K_CACHE, RL_DIGEST_C1, RL_DIGEST_C2}) CHECK(c & 1);
    rl_bucket_digest out[2] = {{7, 7, 7}, {7, 7, 7}}, tot = {7, 7, 7};
    CHECK(rl_limiter_digest(nullptr, 0, 0, 1, 0, out, &tot) == RL_E_INVALID_ARG);
    CHECK(rl_limiter_digest(nullptr, 0, 0, 0, RL_DIGEST_CACHE, nullptr, &tot) == RL_E_INVALID_ARG);
    CHECK(rl_limiter_digest_device(nullptr, 0, 0, 1, 0, out, nullptr) == RL_E_INVALID_ARG);
    CHECK(out[0].entries == 7 && out[1].xr == 7 && tot.sum == 7);
    // one known answer of the restatement (key hash 0, a cache entry; tests/test_digest_model.py)
    CHECK(entryHash(0, RL_DIGEST_K_CACHE, 1700000000400ULL, 0, 0) == 0xfa3d5e6273c94d32ULL);
}

using Store = std::map<std::pair<uint16_t, uint32_t>, std::vector<rl_key_image>>;   // (limiter, bucket)

// snapshotChanged into the store; returns the buckets the sink saw and (zero) those that came empty.
static std::set<uint32_t> checkpoint(GpuEngine& eng, uint16_t id, int64_t nowNanos, uint32_t bits,
                                     const std::vector<rl_bucket_digest>& previous,
                                     std::vector<rl_bucket_digest>* current, Store& store,
                                     std::set<uint32_t>* empty) {
    std::set<uint32_t> seen;
    size_t got = 0;
    const size_t delivered = eng.snapshotChanged(
        id, nowNanos, bits, previous, current, 256, [&](uint32_t b, const rl_key_image* im, size_t n) {
            std::vector<rl_key_image>& chunk = store[{id, b}];
            if (seen.insert(b).second) chunk.clear();      // a changed bucket replaces its chunk
            if (n == 0 && empty) empty->insert(b);
            for (size_t i = 0; i < n; ++i) {
                CHECK(im[i].limiter == id && bucketOf(im[i].key_hash, bits) == b);
                chunk.push_back(im[i]);
            }
            got += n;
        });
    CHECK(delivered == got);
    return seen;
}

static void gpu_tests() {
    constexpr int N = 3000;
    constexpr uint32_t BITS = 3;
    GpuEngine::Options o;
    o.maxBatch = 1 << 16;
    o.defaultCapacity = 1 << 13;
    auto eng = std::make_shared<GpuEngine>(o);
    RateLimitConfig cs;
    cs.maxPermits = 3;
    cs.windowMs = 60000;
    cs.enableLocalCache = true;
    cs.localCacheTtlMs = 5000;
    RateLimitConfig ct;
    ct.maxPermits = 10;
    ct.windowMs = 60000;
    ct.refillRate = 1.0;
    int64_t t_ms = 1700000000000LL / 60000 * 60000 + 30000;      // mid-window
    auto clock = [&] { return t_ms * 1000000; };
    GpuRateLimiter sw(eng, GpuRateLimiter::Algorithm::SlidingWindow, cs, clock);
    GpuRateLimiter tb(eng, GpuRateLimiter::Algorithm::TokenBucket, ct, clock);

    std::vector<std::string> user(N);
    std::vector<uint64_t> hash(N);
    for (int i = 0; i < N; ++i) {
        user[i] = "user-" + std::to_string(i);
        hash[i] = keyHash(user[i]);
    }
    auto batch = [&](GpuRateLimiter& l, const std::vector<uint64_t>& k, const std::vector<int32_t>& p,
                     std::vector<uint8_t>* allowed, std::vector<int64_t>* remaining) {
        const size_t n = k.size();
        std::vector<int64_t> now(n, t_ms * 1000000);
        std::unique_ptr<bool[]> a(new bool[n]);
        std::vector<int64_t> r(n);
        l.tryAcquireBatch(n, k.data(), p.data(), now.data(), a.get(), r.data());
        if (allowed) allowed->assign(a.get(), a.get() + n);
        if (remaining) *remaining = r;
    };
    // user i tries (i % 4) + 1 times against 3 per minute (every fourth ends exhausted, with a
    // rejecting cache entry) and takes (i % 5) + 1 of 10 tokens
    {
        std::vector<uint64_t> k;
        std::vector<int32_t> p;
        for (int i = 0; i < N; ++i)
            for (int j = 0; j <= i % 4; ++j) { k.push_back(hash[i]); p.push_back(1); }
        batch(sw, k, p, nullptr, nullptr);
        k.clear(); p.clear();
        for (int i = 0; i < N; ++i) { k.push_back(hash[i]); p.push_back(i % 5 + 1); }
        batch(tb, k, p, nullptr, nullptr);
    }
    int64_t now = t_ms * 1000000;
    // bad arguments
    CHECK(throws<IllegalArgumentException>([&] { eng->digest(200, now, 0); }));
    CHECK(throws<IllegalArgumentException>([&] { eng->digest(sw.limiterId(), now, 40); }));
    CHECK(throws<IllegalArgumentException>([&] {
        eng->snapshotChanged(sw.limiterId(), now, BITS, std::vector<rl_bucket_digest>(7), nullptr, 256, nullptr);
    }));
    CHECK(throws<IllegalArgumentException>([&] { eng->snapshotChanged(200, now, BITS, {}, nullptr, 256, nullptr); }));

    // the digests against the restatement over the export
    uint64_t slots = 0;
    CHECK(rl_limiter_slots(eng->handle(), sw.limiterId(), &slots) == RL_OK && slots >= 256 * 16);
    uint32_t kbits = 0;                                   // the table's region bits
    while ((slots / 256) >> (kbits + 1)) ++kbits;
    CHECK(throws<IllegalArgumentException>([&] { eng->digest(sw.limiterId(), now, kbits + 1); }));
    for (GpuRateLimiter* l : {&sw, &tb})
        for (uint32_t bits : {0u, BITS, kbits}) {
            const auto got = eng->digest(l->limiterId(), now, bits, false);
            CHECK(same(got, fromExport(eng->handle(), l->limiterId(), now, bits)));
            uint64_t entries = 0;
            for (const auto& d : got) entries += d.entries;
            CHECK(entries == (uint64_t)N);
        }
    {   // the cache entries: as many more as the census counts; none for the token bucket
        const auto with = sw.digest(BITS), without = eng->digest(sw.limiterId(), now, BITS, false);
        CHECK(same(with, eng->digest(sw.limiterId(), now, BITS, true)));
        uint64_t more = 0;
        for (uint32_t b = 0; b < (1u << BITS); ++b) more += with[b].entries - without[b].entries;
        // (a cached count >= maxPermits rejects: the users with three or four tries)
        CHECK(more == sw.usage().cache_blocked && more == (uint64_t)N / 2);
        CHECK(same(tb.digest(BITS), eng->digest(tb.limiterId(), now, BITS, false)));
    }

    // a per-bucket checkpoint of both limiters
    Store store;
    std::vector<rl_bucket_digest> sw1, tb1;
    std::set<uint32_t> empty;
    CHECK(checkpoint(*eng, sw.limiterId(), now, BITS, {}, &sw1, store, &empty).size() == 8);
    CHECK(checkpoint(*eng, tb.limiterId(), now, BITS, {}, &tb1, store, &empty).size() == 8);
    CHECK(empty.empty() && store.size() == 16);
    CHECK(same(sw1, sw.digest(BITS)) && same(tb1, tb.digest(BITS)));
    for (const auto& kv : store) CHECK(kv.second.size() > 256);     // several chunks per bucket

    // 10 ms later: sliding window, one more request of the once-seen users of buckets 2 and 5 and
    // a reset of every user of bucket 6; token bucket, one token of the users of bucket 1 and a
    // reset of every user of bucket 6
    t_ms += 10;
    now = t_ms * 1000000;
    {
        std::vector<uint64_t> k, k1;
        for (int i = 0; i < N; ++i) {
            const uint32_t b = bucketOf(hash[i], BITS);
            if ((b == 2 || b == 5) && i % 4 == 0) k.push_back(hash[i]);
            if (b == 1) k1.push_back(hash[i]);
            if (b == 6) { sw.reset(user[i]); tb.reset(user[i]); }
        }
        CHECK(k.size() > 20 && k1.size() > 100);
        std::vector<uint8_t> a;
        batch(sw, k, std::vector<int32_t>(k.size(), 1), &a, nullptr);
        CHECK(std::count(a.begin(), a.end(), 1) == (long)k.size());
        batch(tb, k1, std::vector<int32_t>(k1.size(), 1), &a, nullptr);
        CHECK(std::count(a.begin(), a.end(), 1) == (long)k1.size());
    }
    std::vector<rl_bucket_digest> sw2, tb2;
    auto differing = [](const std::vector<rl_bucket_digest>& a, const std::vector<rl_bucket_digest>& b) {
        std::set<uint32_t> s;
        for (uint32_t i = 0; i < a.size(); ++i)
            if (!same(a[i], b[i])) s.insert(i);
        return s;
    };
    const auto seenSw = checkpoint(*eng, sw.limiterId(), now, BITS, sw1, &sw2, store, &empty);
    CHECK(seenSw == differing(sw1, sw2) && seenSw == (std::set<uint32_t>{2, 5, 6}));
    CHECK((empty == std::set<uint32_t>{6} && store[{sw.limiterId(), 6}].empty()));
    empty.clear();
    const auto seenTb = checkpoint(*eng, tb.limiterId(), now, BITS, tb1, &tb2, store, &empty);
    CHECK(seenTb == differing(tb1, tb2) && seenTb == (std::set<uint32_t>{1, 6}));
    CHECK((empty == std::set<uint32_t>{6} && store[{tb.limiterId(), 6}].empty()));
    CHECK(sw2[6].entries == 0 && sw2[6].sum == 0 && sw2[6].xr == 0 && tb2[6].entries == 0);
    // nothing changed since: no bucket is delivered
    CHECK(checkpoint(*eng, sw.limiterId(), now, BITS, sw2, nullptr, store, nullptr).empty());

    // the merged checkpoint into a fresh engine of another size
    GpuEngine::Options o2 = o;
    o2.defaultCapacity = 1 << 15;
    auto eng2 = std::make_shared<GpuEngine>(o2);
    GpuRateLimiter swB(eng2, GpuRateLimiter::Algorithm::SlidingWindow, cs, clock);
    GpuRateLimiter tbB(eng2, GpuRateLimiter::Algorithm::TokenBucket, ct, clock);
    CHECK(swB.limiterId() == sw.limiterId() && tbB.limiterId() == tb.limiterId());
    uint64_t slots2 = 0;
    CHECK(rl_limiter_slots(eng2->handle(), swB.limiterId(), &slots2) == RL_OK && slots2 != slots);
    for (const auto& kv : store)
        CHECK(eng2->restore(kv.second.data(), kv.second.size()) == kv.second.size());
    for (uint32_t bits : {0u, BITS, kbits}) {
        CHECK(same(swB.digest(bits), sw.digest(bits)));
        CHECK(same(tbB.digest(bits), tb.digest(bits)));
    }
    CHECK(same(sw.digest(BITS), sw2) && same(tb.digest(BITS), tb2));
    // ... and the same decisions for every key on one further batch
    t_ms += 10;
    std::vector<int32_t> ones(N, 1);
    std::vector<uint8_t> a1, a2;
    std::vector<int64_t> r1, r2;
    batch(sw, hash, ones, &a1, &r1);
    batch(swB, hash, ones, &a2, &r2);
    CHECK(a1 == a2 && r1 == r2);
    CHECK(std::count(a1.begin(), a1.end(), 1) > N / 4 && std::count(a1.begin(), a1.end(), 0) > N / 8);
    batch(tb, hash, std::vector<int32_t>(N, 6), &a1, &r1);
    batch(tbB, hash, std::vector<int32_t>(N, 6), &a2, &r2);
    CHECK(a1 == a2 && r1 == r2);
    CHECK(std::count(a1.begin(), a1.end(), 1) > N / 4 && std::count(a1.begin(), a1.end(), 0) > N / 8);
    CHECK(same(swB.digest(BITS), sw.digest(BITS)) && same(tbB.digest(BITS), tb.digest(BITS)));
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    cpu_tests();
    if (mode == "gpu") gpu_tests();
    std::printf("%s: %s (%d failures)\n", mode.c_str(), failures ? "FAIL" : "ok", failures);
    return failures ? 1 : 0;
}
