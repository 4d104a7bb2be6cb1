// rl_small.hpp — the small-batch path (DESIGN.md §4 "Small batches"): its bound, the rule that
// marks a request invalid, the stable partition of a batch by region that one workgroup does in
// LDS, the hand-out of the touched regions to the workgroup's waves, the scratch sizes and the
// layout of the host form's page-locked block. Plain C++ with no HIP header, every function
// RL_SMALL_HD, so that k_small_batch (rl_small.hip) and a host model share them:
// tests/cpp/test_small_plan.cpp runs the whole partition on the host through these functions,
// in buffers of exactly the sizes stated here, against std::stable_sort.
//
// The partition is a rank by counting. Request i of region g gets the sort key g << 32 | i; its
// position in region order is the number of requests whose key is smaller. Keys are distinct,
// so the positions are a bijection of [0, n), ordered by region and inside a region by arrival:
// the order the per-key contract of rl_engine.h needs. n^2 compares spread over the workgroup's
// threads (n = 1024: 2048 broadcast LDS reads per thread) cost less than the barriers of a
// digit-by-digit partition at these sizes, and no count array depends on the number of regions.
// A sorted position p starts a region's run iff p == 0 or its region differs from p - 1's (its
// head), and ends one iff p == n - 1 or it differs from p + 1's: the heads, ranked by wave
// ballots, are the list of touched regions (RegionArgs::order), rstart / rend their runs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RL_SMALL_HD __host__ __device__
#else
#define RL_SMALL_HD
#endif

namespace rl {

constexpr uint32_t kSmallMax = 1024;          // RL_SMALL_BATCH_MAX
constexpr uint32_t kSmallThreads = 512;       // one workgroup of kSmallWaves waves
constexpr uint32_t kSmallWaves = kSmallThreads / 64;
constexpr uint32_t kSmallPer = kSmallMax / kSmallThreads;   // requests per thread: i = t + k * kSmallThreads
constexpr uint32_t kSmallHeadWaves = kSmallMax / 64;        // waves of sorted positions (head counts)
constexpr uint32_t kSmallPad = 64;            // a region wave's idle lanes write results at n + lane
static_assert(kSmallMax % kSmallThreads == 0 && kSmallThreads % 64 == 0, "whole waves, whole rounds");

// permits <= 0 of an acquire, an unknown limiter, an unknown operation: the request is decided
// RL_REMAINING_INVALID and touches no state (as encode_request, rl_partition.hip).
RL_SMALL_HD inline bool small_invalid(uint32_t n_lim, uint32_t lim, uint32_t op, int32_t permits) {
    return lim >= n_lim || op > 2u || (op == 0u && permits <= 0);
}

RL_SMALL_HD inline uint64_t small_sort_key(uint32_t region, uint32_t i) {
    return (uint64_t)region << 32 | i;
}
// Position of request i in region order: the keys smaller than its own among key[0, n).
RL_SMALL_HD inline uint32_t small_rank(const uint64_t* key, uint32_t n, uint32_t i) {
    const uint64_t mine = key[i];
    uint32_t r = 0;
    for (uint32_t j = 0; j < n; ++j) r += key[j] < mine ? 1u : 0u;
    return r;
}
// reg[p]: the region of sorted position p, p < n.
RL_SMALL_HD inline bool small_head(const uint32_t* reg, uint32_t n, uint32_t p) {
    return p < n && (p == 0 || reg[p - 1] != reg[p]);
}
RL_SMALL_HD inline bool small_tail(const uint32_t* reg, uint32_t n, uint32_t p) {
    return p < n && (p + 1 == n || reg[p + 1] != reg[p]);
}
// Sorted position of thread t in round k, and the wave of sorted positions it belongs to (64
// consecutive positions: one ballot ranks their heads).
RL_SMALL_HD inline uint32_t small_index(uint32_t t, uint32_t k) { return t + k * kSmallThreads; }
RL_SMALL_HD inline uint32_t small_head_wave(uint32_t p) { return p / 64; }
// Entry of the touched list a head writes: the heads of the waves before its own (wcnt, one
// count per wave of sorted positions), plus its rank among its wave's heads (the ballot's bits
// below its lane).
RL_SMALL_HD inline uint32_t small_head_base(const uint32_t* wcnt, uint32_t p) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < small_head_wave(p); ++w) s += wcnt[w];
    return s;
}
// (the kernel takes this count from mbcnt, popc_below)
RL_SMALL_HD inline uint32_t small_bits_below(uint64_t ballot, uint32_t lane) {
    return (uint32_t)__builtin_popcountll(ballot & ((1ULL << (lane & 63u)) - 1));
}
RL_SMALL_HD inline uint32_t small_head_slot(const uint32_t* wcnt, uint32_t p, uint64_t ballot) {
    return small_head_base(wcnt, p) + small_bits_below(ballot, p & 63u);
}
// Wave w decides entries w, w + kSmallWaves, ... of the touched list, one region after the other.
RL_SMALL_HD inline uint32_t small_wave_first(uint32_t w) { return w; }
RL_SMALL_HD inline uint32_t small_wave_step() { return kSmallWaves; }

// Scratch of the path, in elements: records, packed results, escaped remainders and balances
// carry the region waves' padding entries past the batch; rstart / rend are indexed by region;
// the touched list holds its length at [n_regions] (the layout of RegionArgs::order).
RL_SMALL_HD inline size_t small_rec_count() { return kSmallMax + kSmallPad; }
RL_SMALL_HD inline size_t small_region_words(size_t n_regions) { return n_regions; }
RL_SMALL_HD inline size_t small_order_words(size_t n_regions) { return n_regions + 1; }

// The host form's page-locked block: the five request arrays, then the three result arrays,
// each for kSmallMax requests at an offset that is a multiple of its element size.
struct SmallBlock {
    size_t key, now_ns, remaining, tokens, permits, limiter, op, allowed, bytes;
};
RL_SMALL_HD inline SmallBlock small_block() {
    SmallBlock b{};
    size_t at = 0;
    b.key = at;       at += (size_t)kSmallMax * 8;
    b.now_ns = at;    at += (size_t)kSmallMax * 8;
    b.remaining = at; at += (size_t)kSmallMax * 8;
    b.tokens = at;    at += (size_t)kSmallMax * 8;
    b.permits = at;   at += (size_t)kSmallMax * 4;
    b.limiter = at;   at += (size_t)kSmallMax * 2;
    b.op = at;        at += (size_t)kSmallMax;
    b.allowed = at;   at += (size_t)kSmallMax;
    b.bytes = at;
    return b;
}

}  // namespace rl
