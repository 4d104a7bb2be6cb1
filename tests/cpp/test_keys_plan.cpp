// The arithmetic of a string-key batch (csrc/rl_keys.hpp) on the CPU: the offset check and the
// chunk planner against brute force, on seeded random offset arrays and on the edge cases (no
// keys, all-empty keys, a 4096-byte key at a chunk boundary, max_bytes == 4096, decreasing
// offsets, offsets past the end, a 4097-byte key). No engine, no GPU.
#include <cstdio>
#include <vector>

#include "../../distributed-rate-limiter_amd/csrc/rl_keys.hpp"

using namespace rl;

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::printf("FAILED %s (%s:%d)\n", #x, __FILE__, __LINE__);     \
            return 1;                                                       \
        }                                                                   \
    } while (0)

namespace {
uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint64_t mix(uint64_t z) {                          // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
uint64_t rnd() { return mix(rng_state += 0x9E3779B97F4A7C15ULL); }

// the definition of include/rl_engine.h, condition by condition
bool brute_ok(uint64_t o0, uint64_t o1, uint64_t len) {
    if (o0 > o1) return false;
    if (o1 > len) return false;
    uint64_t bytes = 0;
    for (uint64_t p = o0; p < o1 && bytes <= kKeyMaxBytes; ++p) ++bytes;   // count them
    return bytes <= kKeyMaxBytes;
}
size_t brute_first_malformed(const std::vector<uint64_t>& off, uint64_t len) {
    const size_t n = off.size() - 1;
    for (size_t i = 0; i < n; ++i)
        if (!brute_ok(off[i], off[i + 1], len)) return i;
    return n;
}
// the largest m >= 1 with m <= max_keys, at + m <= n and off[at + m] - off[at] <= max_bytes,
// tried one by one from the top
size_t brute_chunk(const std::vector<uint64_t>& off, size_t at, size_t max_keys, uint64_t max_bytes) {
    const size_t n = off.size() - 1;
    size_t m = n - at < max_keys ? n - at : max_keys;
    while (m > 1 && off[at + m] - off[at] > max_bytes) --m;
    return m;
}
std::vector<uint64_t> offsets_of(const std::vector<uint64_t>& lens, uint64_t first) {
    std::vector<uint64_t> off(1, first);
    for (uint64_t l : lens) off.push_back(off.back() + l);
    return off;
}
// every chunk of the batch agrees with brute force, and the chunks tile [0, n)
int check_chunks(const std::vector<uint64_t>& off, size_t max_keys, uint64_t max_bytes) {
    const size_t n = off.size() - 1;
    size_t at = 0, chunks = 0;
    while (at < n) {
        const size_t m = keys_chunk(off.data(), n, at, max_keys, max_bytes);
        CHECK(m >= 1 && m <= max_keys && at + m <= n);
        CHECK(m == brute_chunk(off, at, max_keys, max_bytes));
        CHECK(off[at + m] - off[at] <= max_bytes);
        CHECK(at + m == n || m == max_keys || off[at + m + 1] - off[at] > max_bytes);   // maximal
        at += m;
        CHECK(++chunks <= n);
    }
    CHECK(at == n);
    return 0;
}
}  // namespace

int main() {
    // ---- the offset check
    CHECK(key_well_formed(0, 0, 0));                               // an empty key in an empty blob
    CHECK(key_well_formed(5, 5, 5) && !key_well_formed(6, 6, 5));
    CHECK(key_well_formed(0, 4096, 4096) && !key_well_formed(0, 4097, 4097));   // the length limit
    CHECK(key_well_formed(100, 4196, 5000) && !key_well_formed(100, 4197, 5000));
    CHECK(!key_well_formed(10, 9, 100));                           // decreasing
    CHECK(!key_well_formed(90, 101, 100));                         // past the end
    CHECK(!key_well_formed(~0ULL, 3, 100) && !key_well_formed(3, ~0ULL, 100));   // wrapped (below a bias)
    {
        const uint64_t none[1] = {7};
        CHECK(keys_first_malformed(none, 0, 0) == 0);              // n = 0: nothing to object to
        const std::vector<uint64_t> off = {3, 3, 10, 4106, 4106, 8203, 8203};   // key 4: 4097 bytes
        CHECK(keys_first_malformed(off.data(), 4, 9000) == 4);
        CHECK(keys_first_malformed(off.data(), 6, 9000) == 4);
        CHECK(keys_first_malformed(off.data(), 4, 4105) == 2);     // key 2 ends past the blob
        const std::vector<uint64_t> dec = {0, 8, 4, 12};
        CHECK(keys_first_malformed(dec.data(), 3, 100) == 1);
    }
    for (int round = 0; round < 4000; ++round) {
        const size_t n = rnd() % 40;
        const uint64_t len = rnd() % 20000;
        std::vector<uint64_t> off(n + 1);
        uint64_t o = rnd() % 64;
        for (size_t i = 0; i <= n; ++i) {
            off[i] = o;
            const uint64_t kind = rnd() % 16;
            if (kind == 0 && o) o -= 1 + rnd() % o;                // decreasing
            else if (kind == 1) o += 4090 + rnd() % 16;            // around the length limit
            else if (kind == 2) o = len - rnd() % 4 + rnd() % 8;   // around the end (may wrap below 0)
            else o += rnd() % 300;
        }
        CHECK(keys_first_malformed(off.data(), n, len) == brute_first_malformed(off, len));
        for (size_t i = 0; i < n; ++i)
            CHECK(key_well_formed(off[i], off[i + 1], len) == brute_ok(off[i], off[i + 1], len));
    }

    // ---- the chunk planner
    {
        const std::vector<uint64_t> empty(1, 5);                   // n = 0: no chunk at all
        CHECK(check_chunks(empty, 64, 4096) == 0);
        const std::vector<uint64_t> zeros = offsets_of(std::vector<uint64_t>(1000, 0), 17);   // all-empty keys
        CHECK(check_chunks(zeros, 64, 4096) == 0);
        CHECK(keys_chunk(zeros.data(), 1000, 0, 64, 4096) == 64);
        CHECK(keys_chunk(zeros.data(), 1000, 960, 64, 4096) == 40);
        CHECK(keys_chunk(zeros.data(), 1000, 0, 5000, 4096) == 1000);
        // a 4096-byte key at a chunk boundary, max_bytes == 4096: it is a chunk of its own
        const std::vector<uint64_t> big = offsets_of({100, 3996, 4096, 1, 4095, 4096, 0, 0, 4096}, 9);
        CHECK(check_chunks(big, 64, 4096) == 0);
        CHECK(keys_chunk(big.data(), 9, 0, 64, 4096) == 2);
        CHECK(keys_chunk(big.data(), 9, 2, 64, 4096) == 1);
        CHECK(keys_chunk(big.data(), 9, 3, 64, 4096) == 2);
        CHECK(keys_chunk(big.data(), 9, 5, 64, 4096) == 3);        // 4096 + two empty keys
        CHECK(keys_chunk(big.data(), 9, 8, 64, 4096) == 1);
        CHECK(keys_chunk(big.data(), 9, 0, 1, 1 << 20) == 1);
        CHECK(keys_chunk(big.data(), 9, 0, 64, 1 << 20) == 9);
    }
    for (int round = 0; round < 3000; ++round) {
        const size_t n = 1 + rnd() % 200;
        std::vector<uint64_t> lens(n);
        const uint64_t kind = rnd() % 4;
        for (auto& l : lens)
            l = kind == 0 ? rnd() % 41 : kind == 1 ? rnd() % 4097 : kind == 2 ? (rnd() % 8 ? 0 : 4096) : rnd() % 700;
        const std::vector<uint64_t> off = offsets_of(lens, rnd() % 1000);
        CHECK(keys_first_malformed(off.data(), n, off.back()) == n);
        const size_t max_keys = 1 + rnd() % 70;
        const uint64_t max_bytes = rnd() % 3 == 0 ? 4096 : 4096 + rnd() % 20000;
        CHECK(check_chunks(off, max_keys, max_bytes) == 0);
    }
    std::printf("keys plan: ok\n");
    return 0;
}
