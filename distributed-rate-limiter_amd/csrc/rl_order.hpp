// rl_order.hpp — the digit plan of a stable sort of a batch by time (DESIGN.md §4 "Time order of
// a batch"). Plain C++ with no HIP header; tests/cpp/test_order_plan.cpp checks it on the CPU
// against brute force and sorts by it against std::stable_sort. Nothing in the engine includes
// it yet: every entry point applies a batch in array order.
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

}  // namespace rl
