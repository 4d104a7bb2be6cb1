// The digit plan of a sort of a batch by time (csrc/rl_order.hpp) against brute force: spans 0,
// 1, 2^k - 1, 2^k, 2^k + 1 for every k up to 63 (an int64 clock stays below 2^45), and a radix
// sort driven by the plan on the CPU that must equal std::stable_sort. CPU only. The last line
// prints the plan's constants for tests/test_order_plan.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../distributed-rate-limiter_amd/csrc/rl_order.hpp"

using namespace rl;

namespace {

int g_bad = 0;
#define CHECK(c, ...)                                                     \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (g_bad++ < 20) { std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                 \
    } while (0)

uint32_t brute_bit_length(uint64_t v) {
    for (int b = 63; b >= 0; --b)
        if (v >> b & 1) return (uint32_t)b + 1;
    return 0;
}

void check_plan(uint64_t span) {
    const OrderPlan p = order_plan(span);
    const uint32_t len = brute_bit_length(span);
    CHECK(order_bit_length(span) == len, "span %llu", (unsigned long long)span);
    CHECK(p.passes == (len + 7) / 8, "span %llu passes %u", (unsigned long long)span, p.passes);
    CHECK(p.passes <= kOrderMaxPasses, "span %llu", (unsigned long long)span);
    CHECK((span == 0) == (p.passes == 0), "span %llu", (unsigned long long)span);
    CHECK(p.wide == (len > 32 ? 1u : 0u), "span %llu wide %u", (unsigned long long)span, p.wide);
    if (span < (1ull << 45)) CHECK(p.passes <= kOrderClockPasses, "span %llu", (unsigned long long)span);
    // the digits tile [0, len): contiguous, each 1..8 bits, widths differing by at most one
    uint32_t at = 0, lo = 64, hi = 0;
    for (uint32_t i = 0; i < p.passes; ++i) {
        CHECK(p.shift[i] == at, "span %llu pass %u shift %u", (unsigned long long)span, i, p.shift[i]);
        CHECK(p.bits[i] >= 1 && p.bits[i] <= kOrderDigitBits, "span %llu pass %u bits %u",
              (unsigned long long)span, i, p.bits[i]);
        lo = std::min<uint32_t>(lo, p.bits[i]);
        hi = std::max<uint32_t>(hi, p.bits[i]);
        at += p.bits[i];
    }
    CHECK(at == len, "span %llu covers %u of %u bits", (unsigned long long)span, at, len);
    if (p.passes) CHECK(hi - lo <= 1, "span %llu digits %u..%u", (unsigned long long)span, lo, hi);
}

// A stable LSD sort by the plan's digits equals a stable sort by the whole key.
void check_sort(uint64_t span, std::mt19937_64& rng) {
    const size_t n = 600;
    std::vector<uint64_t> key(n);
    for (auto& k : key) k = span == ~0ull ? rng() : rng() % (span + 1);
    key[0] = 0;
    key[1] = span;
    std::vector<uint32_t> idx(n), tmp(n), want(n);
    for (size_t i = 0; i < n; ++i) idx[i] = want[i] = (uint32_t)i;
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    const OrderPlan p = order_plan(span);
    for (uint32_t ps = 0; ps < p.passes; ++ps) {
        const uint32_t bins = 1u << p.bits[ps];
        std::vector<size_t> start(bins + 1, 0);
        auto digit = [&](uint32_t i) { return (uint32_t)(key[i] >> p.shift[ps]) & (bins - 1); };
        for (uint32_t i : idx) ++start[digit(i) + 1];
        for (uint32_t b = 0; b < bins; ++b) start[b + 1] += start[b];
        for (uint32_t i : idx) tmp[start[digit(i)]++] = i;
        idx.swap(tmp);
    }
    CHECK(idx == want, "span %llu", (unsigned long long)span);
}

}  // namespace

int main() {
    std::mt19937_64 rng(12345);
    std::vector<uint64_t> spans = {0, 1};
    for (int k = 1; k <= 63; ++k)
        for (int64_t d = -1; d <= 1; ++d) spans.push_back((1ull << k) + (uint64_t)d);
    spans.push_back(~0ull);
    for (uint64_t s : spans) {
        check_plan(s);
        check_sort(s, rng);
    }
    for (int i = 0; i < 2000; ++i) check_plan(rng() >> (rng() % 64));
    if (g_bad) {
        std::printf("order plan: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("order plan: ok (%zu spans) digit_bits=%u max_passes=%u clock_passes=%u\n", spans.size(),
                kOrderDigitBits, kOrderMaxPasses, kOrderClockPasses);
    return 0;
}
