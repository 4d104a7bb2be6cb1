// The arithmetic of a batch (csrc/rl_batch_plan.hpp) on the CPU: the digit split, routing, tiles
// and segments over a grid of batch sizes, table sizes and rl_tune values, the k_group tile bound
// against brute-force placements, and points derived by hand. No engine, no device call (the
// constants sit behind the HIP headers, hence the HIP compiler).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../distributed-rate-limiter_amd/csrc/rl_batch_plan.hpp"

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
uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
uint64_t rnd() { return mix(rng_state += 0x9E3779B97F4A7C15ULL); }

BatchTune tune(uint32_t tile_items, uint32_t segments, uint32_t group_bits, bool route, bool hot) {
    BatchTune t;
    t.tile_items = tile_items; t.segments = segments; t.group_bits = group_bits; t.route = route;
    if (!hot) { t.hot_threshold = 0; t.hot_thr_auto = false; }   // as rl_tune("hot_threshold", 0)
    return t;
}

// tiles k_group cuts: a (bin, segment) cell of c records takes ceil(c / tile_recs) of them
uint64_t tiles_of(const std::vector<uint64_t>& cell, uint32_t tile_recs) {
    uint64_t t = 0;
    for (uint64_t c : cell) t += (c + tile_recs - 1) / tile_recs;
    return t;
}
}  // namespace

// what holds for every plan
static int check_plan(const BatchTune& t, size_t n, uint32_t n_regions, const BatchPlan& p) {
    const bool hot = t.hot_threshold > 0;
    // 1. digit split
    CHECK((1ULL << p.bitsP) >= n_regions && (p.bitsP == 1 || (1ULL << (p.bitsP - 1)) < n_regions));
    CHECK((p.passes == 1) == (p.bitsP <= kMaxDigitBits) && (p.passes == 1 || p.passes == 2));
    CHECK(p.dh + p.s0 == p.bitsP && p.dh >= 1 && p.dh <= kMaxDigitBits);
    CHECK(p.s0 >= 0 && p.s0 <= kMaxDigitBits);
    CHECK(p.nb0 <= 1u << kMaxDigitBits);
    // 2. routing
    CHECK(p.hot == hot);
    if (p.route) CHECK(p.passes == 2 && hot && t.route && p.nb0 == (1u << p.dh) + kRouteBins);
    else CHECK(p.nb0 == 1u << p.dh);
    CHECK(p.route || !(hot && t.route && p.passes == 2 && (1u << p.dh) + kRouteBins <= (1u << kMaxDigitBits)));
    CHECK((1u << p.digit_bits) >= p.nb0 && (p.digit_bits == 0 || (1u << (p.digit_bits - 1)) < p.nb0));
    // 3. tiling
    if (t.tile_items) CHECK(p.titems == t.tile_items);
    else CHECK(p.titems == (uint32_t)kTileItems || p.titems == 2u * kTileItems);
    const uint64_t tile_n = (uint64_t)p.titems * kTileThreads;
    CHECK((uint64_t)(p.nt - 1) * tile_n < n && n <= (uint64_t)p.nt * tile_n);
    CHECK((uint64_t)(p.nt_un - 1) * kTile < n && n <= (uint64_t)p.nt_un * kTile);
    CHECK(p.n_segs >= 1 && p.n_segs <= t.segments);
    CHECK((uint64_t)(p.n_segs - 1) * p.seg_tiles < p.nt && p.nt <= (uint64_t)p.n_segs * p.seg_tiles);
    if (p.passes == 1) CHECK(p.n_segs == 1);
    // the scratch the launch chain indexes
    CHECK(p.counts_words == (size_t)p.nb0 * p.nt);
    CHECK(p.seg_words == (p.n_segs > 1 ? (size_t)3 * p.nb0 * p.n_segs : 0));
    if (p.passes == 1) {
        CHECK(p.tile_recs == 0 && p.max_tiles == 0 && p.gtile_words == 0);
    } else {
        const size_t n_bins0 = (size_t)1 << p.dh;
        CHECK(p.tile_recs == group_tile_recs((uint32_t)p.s0));
        // GroupArgs::max_tiles as rl_launch.hpp documents it: full tiles, one partial per cell
        CHECK(p.max_tiles == (n + p.tile_recs - 1) / p.tile_recs + n_bins0 * p.n_segs);
        // tile_base [n_bins0 + 1], tile_bin [max_tiles], tcount [max_tiles][2^s0], then
        // tile_beg / tile_end [max_tiles] each when segmented
        CHECK(p.gtile_words == n_bins0 + 1 + (size_t)p.max_tiles * (1 + ((size_t)1 << p.s0)) +
                                   (p.n_segs > 1 ? (size_t)2 * p.max_tiles : 0));
    }
    // hot threshold, upsweep grid
    CHECK(p.hot_thr == (t.hot_thr_auto ? std::max<uint32_t>(t.hot_threshold, (uint32_t)(n >> 12)) : t.hot_threshold));
    CHECK(p.up_per_cu == (t.up_per_cu ? t.up_per_cu : p.titems > (uint32_t)kTileItems ? 8u : 0u));
    return 0;
}

// 4. no placement of the n records into the (bin, segment) cells needs more tiles than max_tiles
static int check_tile_bound(const BatchPlan& p, size_t n) {
    if (p.passes == 1) return 0;
    const size_t cells = ((size_t)1 << p.dh) * p.n_segs;
    std::vector<uint64_t> c(cells, 0);
    c[rnd() % cells] = n;                                    // all in one cell
    CHECK(tiles_of(c, p.tile_recs) <= p.max_tiles);
    for (size_t i = 0; i < cells; ++i) c[i] = n / cells + (i < n % cells ? 1 : 0);   // one per cell, evenly
    CHECK(tiles_of(c, p.tile_recs) <= p.max_tiles);
    const size_t ones = std::min(n, cells);                  // one per cell, the rest in one
    for (size_t i = 0; i < cells; ++i) c[i] = i < ones ? 1 : 0;
    c[rnd() % ones] += n - ones;
    CHECK(tiles_of(c, p.tile_recs) <= p.max_tiles);
    uint64_t left = n;                                       // a seeded random split
    for (size_t i = 0; i < cells; ++i) {
        const uint64_t take = i + 1 == cells ? left : std::min<uint64_t>(left, rnd() % (2 * n / cells + 2));
        c[i] = take;
        left -= take;
    }
    CHECK(tiles_of(c, p.tile_recs) <= p.max_tiles);
    return 0;
}

static int grid_tests() {
    const size_t ns[] = {1, 511, 512, 65535, 65536, 65537, ((size_t)3 << 26) - 1, (size_t)3 << 26, 0xFFFFFFF0ULL};
    const uint32_t regions[] = {8, 4096, 8192, 8193, 1u << 20, 1u << 24};
    const uint32_t tile_items[] = {0, 8, 1024}, segments[] = {1, 4, 64}, group_bits[] = {1, 12, 13};
    for (size_t n : ns)
        for (uint32_t r : regions)
            for (uint32_t ti : tile_items)
                for (uint32_t sg : segments)
                    for (uint32_t gb : group_bits)
                        for (int route = 0; route < 2; ++route)
                            for (int hot = 0; hot < 2; ++hot) {
                                const BatchTune t = tune(ti, sg, gb, route != 0, hot != 0);
                                BatchPlan p;
                                CHECK(plan_batch(t, n, r, &p) == RL_OK);
                                if (check_plan(t, n, r, p)) return 1;
                                const size_t m = std::min<size_t>(n, (size_t)1 << 20);
                                CHECK(plan_batch(t, m, r, &p) == RL_OK);
                                if (check_plan(t, m, r, p) || check_tile_bound(p, m)) return 1;
                            }
    return 0;
}

// points worked out by hand from run_batch_device as it stood before the plan moved here
static int hand_tests() {
    BatchPlan p;
    const BatchTune d;                                       // an engine's defaults
    CHECK(d.tile_items == 0 && d.segments == 1 && d.group_bits == 12 && d.hot_threshold == 16384 &&
          d.hot_thr_auto && d.route && d.up_per_cu == 0);
    CHECK(plan_batch(d, (size_t)1 << 20, 4096, &p) == RL_OK);
    CHECK(p.passes == 1 && p.dh == 12 && p.s0 == 0 && p.nb0 == 4096 && p.nt == 16 && p.n_segs == 1 && !p.route);
    CHECK(plan_batch(d, (size_t)1 << 20, 1u << 20, &p) == RL_OK);
    CHECK(p.passes == 2 && p.dh == 12 && p.s0 == 8 && p.route && p.nb0 == 5120 && p.digit_bits == 13);
    BatchTune t = d;
    t.group_bits = 13;
    CHECK(plan_batch(t, (size_t)1 << 20, 1u << 20, &p) == RL_OK);
    CHECK(p.passes == 2 && p.dh == 13 && p.s0 == 7 && !p.route && p.nb0 == 8192 && p.digit_bits == 13);
    CHECK(plan_batch(d, (size_t)1 << 20, 1u << 24, &p) == RL_OK);
    CHECK(p.dh == 12 && p.s0 == 12);
    t = d;
    t.group_bits = 1;                                        // the low digit holds at most 13 bits
    CHECK(plan_batch(t, (size_t)1 << 20, 1u << 24, &p) == RL_OK);
    CHECK(p.dh == 11 && p.s0 == 13);
    CHECK(plan_batch(d, (size_t)3 << 26, 4096, &p) == RL_OK);
    CHECK(p.titems == 256 && p.nt == 1536 && p.nt_un == 3072 && p.up_per_cu == 8);
    CHECK(plan_batch(d, ((size_t)3 << 26) - 1, 4096, &p) == RL_OK);
    CHECK(p.titems == 128 && p.nt == 3072 && p.nt_un == 3072 && p.up_per_cu == 0);
    // segments: (nt, segments) -> (seg_tiles, n_segs); tiles of 8 x 512 requests, a two-pass table
    t = d;
    t.tile_items = 8;
    t.segments = 4;
    const uint32_t seg[4][3] = {{10, 3, 4}, {9, 3, 3}, {5, 2, 3}, {1, 1, 1}};
    for (const auto& s : seg) {
        CHECK(plan_batch(t, (size_t)s[0] * 4096, 1u << 20, &p) == RL_OK);
        CHECK(p.nt == s[0] && p.seg_tiles == s[1] && p.n_segs == s[2]);
        CHECK(plan_batch(t, (size_t)s[0] * 4096, 4096, &p) == RL_OK);   // one pass: never segmented
        CHECK(p.nt == s[0] && p.seg_tiles == s[0] && p.n_segs == 1);
    }
    // the hot threshold scales with the batch until it is set
    CHECK(plan_batch(d, (size_t)1 << 28, 4096, &p) == RL_OK && p.hot_thr == 65536 && p.hot);
    CHECK(plan_batch(d, (size_t)1 << 20, 4096, &p) == RL_OK && p.hot_thr == 16384);
    t = d;
    t.hot_threshold = 100; t.hot_thr_auto = false;
    CHECK(plan_batch(t, (size_t)1 << 28, 4096, &p) == RL_OK && p.hot_thr == 100 && p.hot);
    t.hot_threshold = 0;
    CHECK(plan_batch(t, (size_t)1 << 20, 1u << 20, &p) == RL_OK && !p.hot && !p.route && p.nb0 == 4096);
    t = d;
    t.up_per_cu = 3;
    CHECK(plan_batch(t, (size_t)1 << 20, 4096, &p) == RL_OK && p.up_per_cu == 3);
    // more regions than two digits address
    CHECK(plan_batch(d, 1, (1u << 26) + 1, &p) == RL_E_LIMITERS);
    CHECK(plan_batch(d, 1, 1u << 26, &p) == RL_OK && p.dh == 13 && p.s0 == 13);
    return 0;
}

int main() {
    if (hand_tests() || grid_tests()) return 1;
    std::printf("batch plan: ok\n");
    return 0;
}
