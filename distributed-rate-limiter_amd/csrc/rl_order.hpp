// rl_order.hpp — the sort of a batch by time (DESIGN.md §4 "Time order of a batch"): its digit
// plan, and the addressing of a tiled sort that follows it (tile size, tile count, the [bin][tile]
// count index, key and digit, scratch sizes). Plain C++ with no HIP header, every function
// RL_ORDER_HD, so that kernels and a host model can share them. tests/cpp/test_order_plan.cpp
// checks the plan against brute force; tests/cpp/test_order_sort.cpp runs the whole chain (range,
// plan, count, offsets, scatter, gather, return) on the host tile by tile through these functions,
// in buffers of exactly the sizes stated here, against std::stable_sort. Nothing in the engine
// includes this header yet: there is no kernel behind it, and every entry point applies a batch
// in array order.
//
// Time order of a batch is the order by (ms[i], i), ms = floorDiv(now_ns, 1e6): a stable sort by
// millisecond. The sort key is ms - min_ms, an unsigned value of bit_length(span) bits with
// span = max_ms - min_ms. Every int64 now_ns gives |ms| < 2^43.1, so span < 2^44.1: the plan
// takes any 64-bit span and needs at most kOrderClockPasses passes for the spans an int64 clock
// can produce. The plan is that of a least-significant-digit radix sort:
//  * passes = ceil(bit_length(span) / kOrderDigitBits); span 0 gives 0 passes (nothing to sort).
//  * The key's bits are spread evenly over the passes (a 12-bit span sorts in two 6-bit passes,
//    not 8 + 4), least significant digit first; every digit has 1..kOrderDigitBits bits and the
//    digits tile [0, bit_length(span)) exactly.
//  * wide: keys need 64-bit words only when the span needs more than 32 bits.
// A pass cuts the n requests into tiles of kOrderTile, counts every tile's digits into
// counts[bin][tile] (bin-major, always kOrderBins rows), scans every row exclusively (the row
// totals aside), and places element e of tile t at
//   (exclusive scan of the totals)[bin] + counts[bin][t] + (rank of e among t's elements of bin).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RL_ORDER_HD __host__ __device__
#else
#define RL_ORDER_HD
#endif

namespace rl {

constexpr uint32_t kOrderDigitBits = 8;       // widest digit: 256 bins per pass
constexpr uint32_t kOrderMaxPasses = 8;       // 64 key bits
constexpr uint32_t kOrderClockPasses = 6;     // ceil(45 / 8): any span of an int64 nanosecond clock

struct OrderPlan {
    uint32_t passes;                    // digit passes (0: already sorted by construction)
    uint32_t wide;                      // 1: the key needs more than 32 bits
    uint8_t shift[kOrderMaxPasses];     // pass p sorts key bits [shift[p], shift[p] + bits[p])
    uint8_t bits[kOrderMaxPasses];
};

RL_ORDER_HD inline uint32_t order_bit_length(uint64_t v) {
    uint32_t b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

RL_ORDER_HD inline OrderPlan order_plan(uint64_t span_ms) {
    OrderPlan p{};
    const uint32_t len = order_bit_length(span_ms);
    p.passes = (len + kOrderDigitBits - 1) / kOrderDigitBits;
    p.wide = len > 32 ? 1u : 0u;
    uint32_t at = 0;
    for (uint32_t i = 0; i < p.passes; ++i) {
        const uint32_t left = p.passes - i;
        const uint32_t b = (len - at + left - 1) / left;      // the rest, spread evenly
        p.shift[i] = (uint8_t)at;
        p.bits[i] = (uint8_t)b;
        at += b;
    }
    return p;
}

// ---- addressing of a tiled sort by the plan (a kernel chain and its host model share it)
constexpr uint32_t kOrderBins = 1u << kOrderDigitBits;   // rows of the counts, whatever a pass' digit
constexpr uint32_t kOrderThreads = 512;       // requests of a tile ranked together (8 waves)
constexpr uint32_t kOrderRounds = 8;          // rounds of kOrderThreads elements per tile
constexpr uint32_t kOrderTile = kOrderThreads * kOrderRounds;    // 4096 requests
constexpr uint64_t kOrderMaxN = 1ull << 31;   // perm is 32 bits wide
constexpr uint32_t kOrderScanWidth = 256;     // columns a row scan takes per step

RL_ORDER_HD inline uint32_t order_tiles(uint64_t n) {
    return (uint32_t)((n + kOrderTile - 1) / kOrderTile);
}
// index of counts[bin][tile] (bin < kOrderBins, tile < tiles)
RL_ORDER_HD inline size_t order_count_index(uint32_t bin, uint32_t tile, uint32_t tiles) {
    return (size_t)bin * tiles + tile;
}
// words of the counts of n requests
RL_ORDER_HD inline size_t order_count_words(uint64_t n) {
    return (size_t)kOrderBins * order_tiles(n);
}
// steps of a row scan over `tiles` columns
RL_ORDER_HD inline uint32_t order_scan_steps(uint32_t tiles) {
    return (tiles + kOrderScanWidth - 1) / kOrderScanWidth;
}
// ms as an unsigned value that orders like the signed one
RL_ORDER_HD inline uint64_t order_ms_key(int64_t ms) { return (uint64_t)ms ^ 0x8000000000000000ull; }
RL_ORDER_HD inline int64_t order_key_ms(uint64_t k) { return (int64_t)(k ^ 0x8000000000000000ull); }
// the sort key of a request: ms - min_ms (< 2^64 for any two int64)
RL_ORDER_HD inline uint64_t order_key(int64_t ms, int64_t min_ms) {
    return (uint64_t)ms - (uint64_t)min_ms;
}
// digit of `key` in a pass over bits [shift, shift + bits): shift <= 63, 1 <= bits <= kOrderDigitBits
RL_ORDER_HD inline uint32_t order_digit(uint64_t key, uint32_t shift, uint32_t bits) {
    return (uint32_t)(key >> shift) & ((1u << bits) - 1u);
}
// What a pass reads from a control block that a device wrote, clamped before it indexes anything.
RL_ORDER_HD inline uint32_t order_clamp_passes(uint32_t passes) {
    return passes < kOrderMaxPasses ? passes : kOrderMaxPasses;
}
RL_ORDER_HD inline uint32_t order_clamp_bits(uint32_t bits) {
    return bits < 1u ? 1u : bits < kOrderDigitBits ? bits : kOrderDigitBits;
}
RL_ORDER_HD inline uint32_t order_clamp_shift(uint32_t shift) { return shift < 63u ? shift : 63u; }

// Scratch of the sort for `cap` requests, in elements; nothing is padded (lanes past n store
// nothing). Two (uint64 key, uint32 index) sets, the counts and their row totals.
RL_ORDER_HD inline size_t order_key_elems(uint64_t cap) { return (size_t)cap; }
RL_ORDER_HD inline size_t order_idx_elems(uint64_t cap) { return (size_t)cap; }
constexpr size_t kOrderTotalWords = kOrderBins;
// Bytes per request of an ordered batch's scratch: the two sort sets (2 x 12), the gathered
// inputs (key 8, permits 4, now 8, limiter 2, op 1 = 23) and the results in sorted order
// (allowed 1, remaining 8, tokens 8 = 17); the counts add 4 * kOrderBins / kOrderTile = 0.25.
constexpr uint32_t kOrderSortBytes = 2 * (8 + 4);
constexpr uint32_t kOrderGatherBytes = 8 + 4 + 8 + 2 + 1;
constexpr uint32_t kOrderResultBytes = 1 + 8 + 8;
RL_ORDER_HD inline size_t order_sort_scratch_bytes(uint64_t cap) {
    return (size_t)cap * kOrderSortBytes + (order_count_words(cap) + kOrderTotalWords) * sizeof(uint32_t);
}
RL_ORDER_HD inline size_t order_exec_scratch_bytes(uint64_t cap) {
    return order_sort_scratch_bytes(cap) + (size_t)cap * (kOrderGatherBytes + kOrderResultBytes);
}
// Requests the scratch is sized for when a batch of n needs more than it holds: this batch plus
// 1/8 headroom (at least 2^20), capped by max_batch, never below n (ensure_scratch's rule).
RL_ORDER_HD inline uint64_t order_scratch_cap(uint64_t n, uint64_t max_batch) {
    uint64_t want = n + n / 8;
    if (want < (1ull << 20)) want = 1ull << 20;
    if (want > max_batch) want = max_batch;
    return want > n ? want : n;
}

}  // namespace rl
