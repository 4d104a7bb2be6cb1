// The small-batch path's stable partition by region (DESIGN.md §4 "Small batches") run on the
// host: sort keys, ranks, the records' scatter, heads and tails, the head counts per wave of
// sorted positions, the touched list and the hand-out of its entries to the waves, through
// exactly the functions of csrc/rl_small.hpp, thread by thread and round by round as
// k_small_batch does, in buffers of exactly the sizes those functions state. Four region
// patterns at sizes around the wave, the round (the workgroup's thread count) and the bound,
// against std::stable_sort by region. Also the validity rule and the host block's layout.
// CPU only; built once more under the address and undefined-behaviour sanitizers. The last line
// prints the constants for tests/test_small_plan.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../distributed-rate-limiter_amd/csrc/rl_small.hpp"

using namespace rl;

namespace {

int g_bad = 0;
#define CHECK(c, ...)                                                     \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (g_bad++ < 20) { std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                 \
    } while (0)

const char* const kPatterns[] = {"one_region", "all_distinct", "two_alternating", "descending"};

// region of request i among n_regions
uint32_t region_for(int pattern, uint32_t i, uint32_t n, uint32_t n_regions) {
    switch (pattern) {
        case 0: return n_regions - 1;
        case 1: return (i * 7u + 3u) % n_regions;            // distinct while n <= n_regions (7 is odd, n_regions a power of two)
        case 2: return (i & 1u) ? 5u : n_regions - 2;
        default: return n - 1 - i;
    }
}

void run_case(int pattern, uint32_t n) {
    const uint32_t n_regions = 2048;                        // >= kSmallMax: pattern 1 and 3 stay distinct
    std::vector<uint32_t> region(n);
    for (uint32_t i = 0; i < n; ++i) region[i] = region_for(pattern, i, n, n_regions);

    // LDS of the partition and the path's scratch, at their stated sizes (heap blocks of exactly
    // those sizes: the sanitizer sees every access past them)
    std::vector<uint64_t> key(kSmallMax);
    std::vector<uint32_t> reg(kSmallMax), wcnt(kSmallHeadWaves);
    std::vector<uint32_t> rec(small_rec_count(), 0xFFFFFFFFu);       // a record = its arrival index here
    std::vector<uint32_t> rstart(small_region_words(n_regions), 0xA5A5A5A5u), rend(small_region_words(n_regions), 0xA5A5A5A5u);
    std::vector<uint32_t> order(small_order_words(n_regions), 0xA5A5A5A5u);
    std::vector<uint32_t> pos(n);

    // phase 1: every thread's requests, round by round
    for (uint32_t k = 0; k < kSmallPer; ++k)
        for (uint32_t t = 0; t < kSmallThreads; ++t) {
            const uint32_t i = small_index(t, k);
            if (i < n) key[i] = small_sort_key(region[i], i);
        }
    // phase 2: ranks, scatter
    for (uint32_t k = 0; k < kSmallPer; ++k)
        for (uint32_t t = 0; t < kSmallThreads; ++t) {
            const uint32_t i = small_index(t, k);
            if (i >= n) continue;
            pos[i] = small_rank(key.data(), n, i);
            CHECK(pos[i] < n, "rank %u of %u", pos[i], n);
            reg[pos[i]] = region[i];
            rec[pos[i]] = i;
        }
    // heads and tails per wave of sorted positions; the ballot of a wave, bit by lane
    std::vector<uint64_t> ballot(kSmallHeadWaves, 0);
    for (uint32_t k = 0; k < kSmallPer; ++k)
        for (uint32_t t = 0; t < kSmallThreads; ++t) {
            const uint32_t p = small_index(t, k);
            if (small_head(reg.data(), n, p)) ballot[small_head_wave(p)] |= 1ULL << (p & 63u);
        }
    for (uint32_t w = 0; w < kSmallHeadWaves; ++w) wcnt[w] = (uint32_t)__builtin_popcountll(ballot[w]);
    uint32_t tot = 0;
    for (uint32_t k = 0; k < kSmallPer; ++k)
        for (uint32_t t = 0; t < kSmallThreads; ++t) {
            const uint32_t p = small_index(t, k);
            if (small_head(reg.data(), n, p)) {
                rstart[reg[p]] = p;
                order[small_head_slot(wcnt.data(), p, ballot[small_head_wave(p)])] = reg[p];
                ++tot;
            }
            if (small_tail(reg.data(), n, p)) rend[reg[p]] = p + 1;
        }
    order[n_regions] = tot;

    // ---- against std::stable_sort by region
    std::vector<uint32_t> ref(n);
    for (uint32_t i = 0; i < n; ++i) ref[i] = i;
    std::stable_sort(ref.begin(), ref.end(), [&](uint32_t a, uint32_t b) { return region[a] < region[b]; });
    for (uint32_t p = 0; p < n; ++p) {
        CHECK(rec[p] == ref[p], "%s n=%u: position %u holds %u, want %u", kPatterns[pattern], n, p, rec[p], ref[p]);
        CHECK(pos[ref[p]] == p, "%s n=%u: pos", kPatterns[pattern], n);
    }
    for (size_t p = n; p < rec.size(); ++p) CHECK(rec[p] == 0xFFFFFFFFu, "record written past n");
    // runs and the touched list: every distinct region once, ascending, with its run
    std::vector<uint32_t> distinct(region);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    CHECK(order[n_regions] == distinct.size(), "%s n=%u: %u touched, want %zu", kPatterns[pattern], n, order[n_regions], distinct.size());
    uint32_t covered = 0;
    for (uint32_t g = 0; g < order[n_regions] && g < distinct.size(); ++g) {
        const uint32_t r = order[g];
        CHECK(r == distinct[g], "%s n=%u: list[%u]", kPatterns[pattern], n, g);
        CHECK(rstart[r] == covered && rend[r] > rstart[r] && rend[r] <= n, "%s n=%u: run of region %u", kPatterns[pattern], n, r);
        for (uint32_t p = rstart[r]; p < rend[r] && p < n; ++p) CHECK(region[rec[p]] == r, "run holds another region");
        covered = rend[r];
    }
    CHECK(covered == n, "%s n=%u: runs cover %u", kPatterns[pattern], n, covered);
    // untouched regions' entries stay as they were
    for (uint32_t r = 0; r < n_regions; ++r)
        if (!std::binary_search(distinct.begin(), distinct.end(), r))
            CHECK(rstart[r] == 0xA5A5A5A5u && rend[r] == 0xA5A5A5A5u, "region %u written", r);
    // the waves take every entry of the list exactly once
    std::vector<uint32_t> taken(tot, 0);
    for (uint32_t w = 0; w < kSmallWaves; ++w)
        for (uint32_t g = small_wave_first(w); g < tot; g += small_wave_step()) ++taken[g];
    for (uint32_t g = 0; g < tot; ++g) CHECK(taken[g] == 1, "entry %u taken %u times", g, taken[g]);
}

}  // namespace

int main() {
    const uint32_t sizes[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, kSmallMax - 1, kSmallMax};
    int cases = 0;
    for (int pat = 0; pat < 4; ++pat)
        for (uint32_t n : sizes) { run_case(pat, n); ++cases; }

    // the validity rule (the upsweep's)
    CHECK(!small_invalid(2, 1, 0, 1) && !small_invalid(2, 0, 1, 0) && !small_invalid(2, 0, 2, -4), "valid");
    CHECK(small_invalid(2, 2, 0, 1) && small_invalid(2, 0, 0, 0) && small_invalid(2, 0, 0, -1) && small_invalid(2, 0, 3, 1),
          "invalid");
    CHECK(small_invalid(0, 0, 0, 1), "no limiter");
    // the host block: every array inside it, aligned to its element, none overlapping
    const SmallBlock b = small_block();
    const size_t off[] = {b.key, b.now_ns, b.remaining, b.tokens, b.permits, b.limiter, b.op, b.allowed};
    const size_t el[] = {8, 8, 8, 8, 4, 2, 1, 1};
    size_t end = 0;
    for (int i = 0; i < 8; ++i) {
        CHECK(off[i] % el[i] == 0 && off[i] >= end, "array %d at %zu", i, off[i]);
        end = off[i] + el[i] * kSmallMax;
    }
    CHECK(end == b.bytes && b.bytes == (size_t)kSmallMax * 40, "block of %zu bytes", b.bytes);
    CHECK(small_rec_count() == kSmallMax + 64 && small_order_words(8) == 9, "scratch sizes");

    if (g_bad) { std::printf("small plan: %d FAILED\n", g_bad); return 1; }
    std::printf("small plan: ok (%d cases) max=%u threads=%u waves=%u per=%u block_bytes=%zu\n", cases, kSmallMax,
                kSmallThreads, kSmallWaves, kSmallPer, b.bytes);
    return 0;
}
