// A stable radix sort of a batch by time (DESIGN.md §4 "Time order of a batch") run on the host:
// range, plan, and per pass count, offsets and scatter tile by tile, then gather and return,
// through exactly the addressing helpers of csrc/rl_order.hpp, in buffers of exactly the sizes
// those helpers give a batch of n with max_batch = n (no headroom, no padding). Every pattern of
// tests/order_cases.py PATTERNS (generated here under the same names) at sizes around the wave,
// the tile's thread count and the tile, plus the smallest n whose row scan takes two steps,
// against std::stable_sort. CPU only; built once more under the address and undefined-behaviour
// sanitizers. The last line prints the addressing constants for tests/test_order_sort.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
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

constexpr int64_t kT0Ms = 1700000000000LL;

int64_t floor_div_ms(int64_t ns) {                     // (rl_device.hpp)
    int64_t q = ns / 1000000;
    if ((ns % 1000000) != 0 && ns < 0) q -= 1;
    return q;
}

const char* const kPatterns[] = {"sorted", "reversed", "equal", "runs2", "runs4", "runs8", "runs64", "random",
                                 "span0", "span255", "span256", "span257", "span65535", "span65536",
                                 "span65537", "span2p32", "straddle0", "same_ms_pairs"};

std::vector<int64_t> runs_ms(std::mt19937_64& rng, size_t n, size_t k, int64_t span) {
    std::vector<int64_t> ms;
    for (size_t i = 0; i < k; ++i) {
        const size_t sz = n / k + (i < n % k ? 1 : 0);
        std::vector<int64_t> run(sz);
        for (auto& v : run) v = (int64_t)(rng() % (uint64_t)(span + 1));
        std::sort(run.begin(), run.end());
        ms.insert(ms.end(), run.begin(), run.end());
    }
    return ms;
}

std::vector<int64_t> with_span(std::mt19937_64& rng, size_t n, int64_t span) {
    std::vector<int64_t> ms(n);
    for (auto& v : ms) v = (int64_t)(rng() % (uint64_t)(span + 1));
    if (n >= 2) {
        const size_t i = rng() % n;
        size_t j = rng() % (n - 1);
        if (j >= i) ++j;
        ms[i] = 0;
        ms[j] = span;
    }
    return ms;
}

std::vector<int64_t> pattern_ns(const std::string& name, size_t n, std::mt19937_64& rng) {
    std::vector<int64_t> ms(n), sub(n);
    for (auto& v : sub) v = (int64_t)(rng() % 1000000);
    auto shift = [&](int64_t by) { for (auto& v : ms) v += by; };
    if (name == "sorted" || name == "reversed") {
        ms = runs_ms(rng, n, 1, 3499);
        if (name == "reversed") std::reverse(ms.begin(), ms.end());
        shift(kT0Ms);
    } else if (name == "equal" || name == "span0") {
        std::fill(ms.begin(), ms.end(), kT0Ms + 17);
    } else if (name.rfind("runs", 0) == 0) {
        ms = runs_ms(rng, n, (size_t)std::stoul(name.substr(4)), 3500);
        shift(kT0Ms);
    } else if (name == "random") {
        for (auto& v : ms) v = (int64_t)(rng() % 100000) + kT0Ms;
    } else if (name == "span2p32") {
        ms = with_span(rng, n, (1LL << 32) + 5);
        shift(kT0Ms);
    } else if (name.rfind("span", 0) == 0) {
        ms = with_span(rng, n, std::stoll(name.substr(4)));
        shift(kT0Ms);
    } else if (name == "straddle0") {
        std::vector<int64_t> ns(n);
        for (auto& v : ns) v = (int64_t)(rng() % 80000000) - 40000000;
        if (n >= 2) { ns[0] = -1; ns[1] = 0; }
        return ns;
    } else if (name == "same_ms_pairs") {
        for (size_t i = 0; i < n; i += 2) {
            ms[i] = (int64_t)(rng() % 50) + kT0Ms;
            if (i + 1 < n) ms[i + 1] = ms[i];
        }
        for (size_t i = 0; i < n; ++i) sub[i] = i % 2 == 0 ? 900000 : 100;
    } else {
        CHECK(false, "unknown pattern %s", name.c_str());
    }
    std::vector<int64_t> ns(n);
    for (size_t i = 0; i < n; ++i) ns[i] = ms[i] * 1000000 + sub[i];
    return ns;
}

// What the range and plan steps leave for the passes (a control block on a device).
struct Ctl {
    uint64_t max_key = 0, inv_min_key = 0, descents = 0;
    uint32_t passes = 0;
    uint8_t shift[kOrderMaxPasses] = {}, bits[kOrderMaxPasses] = {};
};

struct Sorter {
    size_t n;
    uint32_t tiles;
    std::vector<uint64_t> key[2];
    std::vector<uint32_t> idx[2];
    std::vector<uint32_t> counts, totals;
    Ctl ctl;
    uint64_t hdr[4] = {7, 7, 7, 7};

    explicit Sorter(size_t n_) : n(n_), tiles(order_tiles(n_)) {
        const uint64_t cap = order_scratch_cap(n, n);                 // max_batch = n: no headroom
        CHECK(cap == n, "cap %llu", (unsigned long long)cap);
        for (int k = 0; k < 2; ++k) { key[k].resize(order_key_elems(cap)); idx[k].resize(order_idx_elems(cap)); }
        counts.resize(order_count_words(cap));
        totals.resize(kOrderTotalWords);
    }

    void range(const std::vector<int64_t>& ns) {
        for (size_t i = 0; i < n; ++i) {
            const int64_t ms = floor_div_ms(ns[i]);
            const uint64_t k = order_ms_key(ms);
            ctl.max_key = std::max(ctl.max_key, k);
            ctl.inv_min_key = std::max(ctl.inv_min_key, ~k);
            if (i > 0 && ms < floor_div_ms(ns[i - 1])) ++ctl.descents;
        }
    }
    void plan() {
        const uint64_t min_key = ~ctl.inv_min_key;
        const OrderPlan pl = order_plan(ctl.max_key - min_key);
        ctl.passes = ctl.descents ? order_clamp_passes(pl.passes) : 0;
        std::memcpy(ctl.shift, pl.shift, sizeof ctl.shift);
        std::memcpy(ctl.bits, pl.bits, sizeof ctl.bits);
        hdr[0] = ctl.descents;
        hdr[1] = (uint64_t)order_key_ms(min_key);
        hdr[2] = (uint64_t)order_key_ms(ctl.max_key);
        hdr[3] = ctl.passes;
    }
    void load(const std::vector<int64_t>& ns, uint32_t p, uint32_t i, uint64_t& k, uint32_t& x) const {
        if (p == 0) {
            k = order_key(floor_div_ms(ns[i]), order_key_ms(~ctl.inv_min_key));
            x = i;
        } else {
            k = key[p & 1].at(i);
            x = idx[p & 1].at(i);
        }
    }
    // one pass: false when it returns at once (p >= passes)
    bool pass(const std::vector<int64_t>& ns, uint32_t p) {
        const uint32_t passes = order_clamp_passes(ctl.passes);
        if (p >= passes) return false;
        const uint32_t shift = order_clamp_shift(ctl.shift[p]), bits = order_clamp_bits(ctl.bits[p]);
        // count
        for (uint32_t tile = 0; tile < tiles; ++tile) {
            uint32_t hist[kOrderBins] = {};
            for (uint32_t r = 0; r < kOrderRounds; ++r)
                for (uint32_t t = 0; t < kOrderThreads; ++t) {
                    const uint32_t i = tile * kOrderTile + r * kOrderThreads + t;
                    if (i >= n) continue;
                    uint64_t k;
                    uint32_t x;
                    load(ns, p, i, k, x);
                    ++hist[order_digit(k, shift, bits)];
                }
            for (uint32_t b = 0; b < kOrderBins; ++b) counts.at(order_count_index(b, tile, tiles)) = hist[b];
        }
        // offsets: every row in steps of kOrderScanWidth columns
        for (uint32_t b = 0; b < kOrderBins; ++b) {
            uint32_t carry = 0;
            for (uint32_t s = 0; s < order_scan_steps(tiles); ++s) {
                uint32_t run = 0;
                for (uint32_t t = 0; t < kOrderScanWidth; ++t) {
                    const uint32_t col = s * kOrderScanWidth + t;
                    if (col >= tiles) continue;
                    uint32_t& c = counts.at(order_count_index(b, col, tiles));
                    const uint32_t v = c;
                    c = carry + run;
                    run += v;
                }
                carry += run;
            }
            totals.at(b) = carry;
        }
        // scatter
        const bool keep_keys = p + 1 < passes;
        for (uint32_t tile = 0; tile < tiles; ++tile) {
            uint32_t cur[kOrderBins], base = 0;
            for (uint32_t b = 0; b < kOrderBins; ++b) {
                cur[b] = base + counts.at(order_count_index(b, tile, tiles));
                base += totals.at(b);
            }
            for (uint32_t r = 0; r < kOrderRounds; ++r)
                for (uint32_t t = 0; t < kOrderThreads; ++t) {       // (round, wave, lane) = array order
                    const uint32_t i = tile * kOrderTile + r * kOrderThreads + t;
                    if (i >= n) continue;
                    uint64_t k;
                    uint32_t x;
                    load(ns, p, i, k, x);
                    const uint32_t pos = cur[order_digit(k, shift, bits)]++;
                    CHECK(pos < n, "pass %u pos %u n %zu", p, pos, n);
                    if (pos >= n) continue;
                    if (keep_keys) key[(p + 1) & 1].at(pos) = k;
                    idx[(p + 1) & 1].at(pos) = x;
                }
        }
        return true;
    }
    uint32_t perm_at(uint32_t j) const {                              // set passes & 1, or the identity
        const uint32_t passes = order_clamp_passes(ctl.passes);
        return passes == 0 ? j : idx[passes & 1].at(j);
    }
};

uint32_t brute_passes(uint64_t span) {
    uint32_t len = 0;
    while (span) { ++len; span >>= 1; }
    return (len + 7) / 8;
}

void check_case(const std::string& name, size_t n, std::mt19937_64& rng) {
    const std::vector<int64_t> ns = pattern_ns(name, n, rng);
    Sorter s(n);
    if (n == 0) return;                                               // (the host writes the zero header)
    s.range(ns);
    s.plan();
    uint32_t ran = 0;
    for (uint32_t p = 0; p < kOrderClockPasses; ++p) ran += s.pass(ns, p) ? 1 : 0;
    CHECK(ran == s.ctl.passes, "%s n %zu ran %u of %u", name.c_str(), n, ran, s.ctl.passes);
    // the model: std::stable_sort by ms, and the header
    std::vector<uint32_t> want(n);
    for (size_t i = 0; i < n; ++i) want[i] = (uint32_t)i;
    std::stable_sort(want.begin(), want.end(),
                     [&](uint32_t a, uint32_t b) { return floor_div_ms(ns[a]) < floor_div_ms(ns[b]); });
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    uint64_t desc = 0;
    for (size_t i = 0; i < n; ++i) {
        const int64_t ms = floor_div_ms(ns[i]);
        mn = std::min(mn, ms);
        mx = std::max(mx, ms);
        if (i && ms < floor_div_ms(ns[i - 1])) ++desc;
    }
    CHECK(s.hdr[0] == desc && s.hdr[1] == (uint64_t)mn && s.hdr[2] == (uint64_t)mx, "%s n %zu header", name.c_str(), n);
    CHECK(s.hdr[3] == (desc ? brute_passes((uint64_t)mx - (uint64_t)mn) : 0), "%s n %zu passes %llu", name.c_str(), n,
          (unsigned long long)s.hdr[3]);
    size_t wrong = 0;
    for (size_t j = 0; j < n; ++j) wrong += s.perm_at((uint32_t)j) != want[j];
    CHECK(wrong == 0, "%s n %zu: %zu positions differ", name.c_str(), n, wrong);
    // gather and return on arrays of exactly n: X[perm] into g, a result per sorted request, and
    // every result back at perm[j]
    std::vector<uint64_t> x(n), g(n), res(n), out(n, ~0ull);
    for (size_t i = 0; i < n; ++i) x[i] = 0x9e3779b97f4a7c15ull * (i + 1);
    for (size_t j = 0; j < n; ++j) {
        const uint32_t i = s.perm_at((uint32_t)j);
        if (i < n) g.at(j) = x.at(i);
    }
    for (size_t j = 0; j < n; ++j) res[j] = g[j] ^ 0x55;
    for (size_t j = 0; j < n; ++j) {
        const uint32_t i = s.perm_at((uint32_t)j);
        if (i < n) out.at(i) = res.at(j);
    }
    size_t lost = 0;
    for (size_t i = 0; i < n; ++i) lost += out[i] != (x[i] ^ 0x55);
    CHECK(lost == 0, "%s n %zu: %zu results misplaced", name.c_str(), n, lost);
}

}  // namespace

int main() {
    std::mt19937_64 rng(20240607);
    const size_t T = kOrderTile;
    const size_t sizes[] = {0, 1, 2, 63, 64, 65, 511, 512, 513, T - 1, T, T + 1, 2 * T + 17, 40 * T + 3};
    size_t cases = 0;
    for (const char* name : kPatterns)
        for (size_t n : sizes) {
            check_case(name, n, rng);
            ++cases;
        }
    // the smallest n whose row scan takes two steps
    const size_t two_steps = (size_t)kOrderScanWidth * T + 1;
    CHECK(order_scan_steps(order_tiles(two_steps)) == 2 && order_scan_steps(order_tiles(two_steps - 1)) == 1, "scan steps");
    check_case("runs8", two_steps, rng);
    ++cases;
    // the sizing rule
    CHECK(order_scratch_cap(5, 1u << 22) == (1u << 20) && order_scratch_cap(5, 100) == 100 &&
          order_scratch_cap(200, 100) == 200 && order_scratch_cap(1u << 21, 1u << 22) == (1u << 21) + (1u << 18) &&
          order_scratch_cap(1u << 22, 1u << 22) == (1u << 22), "scratch cap");
    CHECK(order_tiles(0) == 0 && order_tiles(1) == 1 && order_tiles(T) == 1 && order_tiles(T + 1) == 2 &&
          order_tiles(kOrderMaxN) == kOrderMaxN / T, "tiles");
    CHECK(order_sort_scratch_bytes(T) == T * 24 + (256 + 256) * 4 &&
          order_exec_scratch_bytes(T) == order_sort_scratch_bytes(T) + T * 40, "scratch bytes");
    if (g_bad) {
        std::printf("order sort: %d checks failed\n", g_bad);
        return 1;
    }
    std::printf("order sort: ok (%zu cases) tile=%u threads=%u rounds=%u bins=%u scan_width=%u two_step_n=%zu "
                "sort_bytes=%u gather_bytes=%u result_bytes=%u\n",
                cases, kOrderTile, kOrderThreads, kOrderRounds, kOrderBins, kOrderScanWidth, two_steps,
                kOrderSortBytes, kOrderGatherBytes, kOrderResultBytes);
    return 0;
}
