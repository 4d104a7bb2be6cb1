// rl_shrink.hpp — the arithmetic of a table shrink (rl_shrink_plan / rl_shrink_limiter; kernels
// in rl_shrink.hip, host side in rl_engine_state.cpp). Plain C++ with no HIP header, so
// tests/cpp/test_shrink_plan.cpp checks it on the CPU against brute force; the engine calls the
// same functions.
//
// A table of 2^k regions halved i times has 2^(k-i) regions, and its region r' holds exactly
// the keys of regions r' << i ... (r' << i) + 2^i - 1 of the table as it is (a region is the k
// bits of the tag below the shard bits, so one bit less merges neighbours: the inverse of
// k_grow's split). The plan counts the slots live at `now` per region, sums them pairwise level
// by level and takes each level's maximum: fullest[i]. Two rules live here.
//  * The halvings: j is the largest i < levels with
//        fullest[i] <= kShrinkFillMax  and  slots_before >> i >= shrink_min_slots(min_keys).
//    i = 0 ("leave the table alone") is always allowed. kShrinkFillMax = kGrowUsed / 2
//    (static_assert in rl_engine_state.cpp): the fullest region of a shrunk table must double its
//    keys before a batch flags the limiter for growth again. shrink_min_slots is the load
//    <= 0.5 rule of rl_grow_limiter with the minimum of one bin (8 regions) per limiter.
//  * The passes: one wave merges at most 2^kShrinkPassBits = 8 source regions (64 KB) into one
//    destination region, so j halvings run as ceil(j / 3) passes through intermediate tables,
//    3 halvings each and the remainder last. Every table is at most 1/8 of the one before
//    (but for the last), so all passes together move at most 8/7 of the first one's bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rl {

constexpr uint32_t kShrinkFillMax = 104;         // RL_SHRINK_FILL_MAX
constexpr uint32_t kShrinkLevels = 24;           // RL_SHRINK_LEVELS
constexpr uint32_t kShrinkRegionSlots = 256;     // kRegionSlots
constexpr uint32_t kShrinkMinRegionBits = 3;     // kBinShift: every limiter keeps >= 8 regions
constexpr uint32_t kShrinkPassBits = 3;          // halvings per merge pass

// valid entries of fullest[] for a table of 2^region_bits regions
inline uint32_t shrink_levels(int region_bits) {
    if (region_bits < (int)kShrinkMinRegionBits) return 1;
    const uint32_t l = (uint32_t)region_bits - kShrinkMinRegionBits + 1;
    return l < kShrinkLevels ? l : kShrinkLevels;
}

// fewest slots the limiter may keep: max(2 * ceil(min_keys / shard_count), 8 * 256)
inline uint64_t shrink_min_slots(uint64_t min_keys, uint32_t shard_count) {
    const uint64_t g = shard_count ? shard_count : 1;
    const uint64_t per_shard = min_keys / g + (min_keys % g ? 1 : 0);
    const uint64_t floor_slots = (uint64_t)kShrinkRegionSlots << kShrinkMinRegionBits;
    if (per_shard > (~0ull >> 1)) return ~0ull;              // (2 * per_shard would wrap)
    return per_shard * 2 > floor_slots ? per_shard * 2 : floor_slots;
}

inline bool shrink_level_ok(uint32_t fullest_i, uint64_t slots_i, uint64_t min_slots) {
    return fullest_i <= kShrinkFillMax && slots_i >= min_slots;
}

inline uint32_t shrink_halvings(const uint32_t* fullest, uint32_t levels, uint64_t slots_before,
                                uint64_t min_keys, uint32_t shard_count) {
    const uint64_t min_slots = shrink_min_slots(min_keys, shard_count);
    uint32_t j = 0;
    for (uint32_t i = 1; i < levels && i < kShrinkLevels; ++i)
        if (shrink_level_ok(fullest[i], slots_before >> i, min_slots)) j = i;
    return j;
}

// the merge passes of j halvings
inline uint32_t shrink_passes(uint32_t j) { return (j + kShrinkPassBits - 1) / kShrinkPassBits; }
inline uint32_t shrink_pass_bits(uint32_t j, uint32_t pass) {
    const uint32_t done = pass * kShrinkPassBits;
    if (done >= j) return 0;
    return j - done < kShrinkPassBits ? j - done : kShrinkPassBits;
}

}  // namespace rl
