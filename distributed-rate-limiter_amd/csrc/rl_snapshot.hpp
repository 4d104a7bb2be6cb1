// rl_snapshot.hpp — the arithmetic of a whole-table snapshot and of an ordered put
// (rl_snapshot_keys / rl_put_keys_device; kernels in rl_snapshot.hip, host side in rl_engine_state.cpp).
// Plain C++ with no HIP header, so tests/cpp/test_snapshot_plan.cpp checks it on the CPU against
// brute force; the kernels and the engine call the same functions.
//
// Two rules live here.
//  * The cut: a snapshot call writes whole regions only. With c[r] the image count of the r-th
//    region of the call's range and o[r] = c[0] + ... + c[r-1], region r is written iff
//    o[r] + c[r] <= cap. The counts are not negative, so the written regions are a prefix of
//    the range: regions_done = their number, n_out = the sum of their counts. If the range is
//    not empty and not even its first region fits, the call is too large and reports c[0].
//  * Ordered form: image i is bound for d(i) = (limiter, region of its tag in that limiter's
//    table). A put takes the images as runs of equal d, one wave per run, which is right iff
//    no d comes back after it has ended, i.e. iff d is non-decreasing. A region is the k bits
//    of the tag below the shard bits (region_local, rl_device.hpp; snap_region_of is the same
//    expression, kept here so that it can be checked without a device), hence for k' <= k
//    region_k' = region_k >> (k - k'): images in the region order of a 2^k-region table are in
//    the region order of every table with the same shard bits and at most as many regions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RL_SNAP_HD __host__ __device__
#else
#define RL_SNAP_HD
#endif

namespace rl {

constexpr uint32_t kSnapRegionSlots = 256;       // RL_SNAPSHOT_MIN_CAP = kRegionSlots
// Regions one snapshot call handles (a longer range is answered in part: regions_done says how
// far). 2^16 regions hold at most 2^24 images, so 32-bit offsets are safe, and the call's
// scratch (a count and an offset per region) is 512 KiB whatever the table's size.
constexpr uint32_t kSnapMaxRegions = 1u << 16;
constexpr uint64_t kSnapMaxImages = 1ull << 31;  // cap (snapshot) and n (put) are bounded by it

// ------------------------------------------------------------------ the cut
RL_SNAP_HD inline bool snap_fits(uint64_t offset, uint32_t count, uint64_t cap) {
    return offset + count <= cap;
}

// The header of a snapshot call over m regions (after clipping) of which the first `fit` ones,
// holding `images` images, fit: { n_out, regions_done, regions_total, 0 }, or the too-large
// case { 0, 0, regions_total, first region's count }.
RL_SNAP_HD inline bool snap_too_large(uint64_t m, uint64_t fit) { return m != 0 && fit == 0; }
RL_SNAP_HD inline void snap_header(uint64_t m, uint64_t fit, uint64_t images, uint32_t first_count,
                                   uint64_t regions_total, uint64_t hdr[4]) {
    const bool big = snap_too_large(m, fit);
    hdr[0] = big ? 0 : images;
    hdr[1] = big ? 0 : fit;
    hdr[2] = regions_total;
    hdr[3] = big ? first_count : 0;
}

// The whole rule from the counts, as the kernels apply it region by region.
inline void snap_cut(const uint32_t* count, uint64_t m, uint64_t cap, uint64_t regions_total,
                     uint64_t hdr[4]) {
    uint64_t off = 0, fit = 0, images = 0;
    for (uint64_t r = 0; r < m; ++r) {
        if (snap_fits(off, count[r], cap)) { ++fit; images += count[r]; }
        off += count[r];
    }
    snap_header(m, fit, images, m ? count[0] : 0u, regions_total, hdr);
}

// The regions [begin, begin + count) clipped to a table of `total` regions and to the per-call
// bound: how many the call handles.
RL_SNAP_HD inline uint64_t snap_clip(uint64_t begin, uint64_t count, uint64_t total) {
    if (begin >= total) return 0;
    uint64_t m = total - begin;
    if (count < m) m = count;
    return m < kSnapMaxRegions ? m : kSnapMaxRegions;
}

// ------------------------------------------------------------------ ordered form
RL_SNAP_HD inline uint32_t snap_region_of(uint64_t tag, int shard_bits, int k) {
    if (k == 0) return 0;
    return (uint32_t)((tag << shard_bits) >> (64 - k));
}
RL_SNAP_HD inline uint64_t snap_dest(uint32_t limiter, uint32_t region) {
    return (uint64_t)limiter << 32 | region;
}
RL_SNAP_HD inline uint64_t snap_dest_of(uint32_t limiter, uint64_t tag, int shard_bits, int region_bits) {
    return snap_dest(limiter, snap_region_of(tag, shard_bits, region_bits));
}
// image i (destination d, its predecessor's d_prev; `first`: i == 0) breaks ordered form /
// starts a run
RL_SNAP_HD inline bool snap_out_of_order(bool first, uint64_t d_prev, uint64_t d) {
    return !first && d < d_prev;
}
RL_SNAP_HD inline bool snap_run_head(bool first, uint64_t d_prev, uint64_t d) {
    return first || d != d_prev;
}

// rejected bits of rl_put_keys_device's header
constexpr uint32_t kPutRejectOrder = 1u;         // not in ordered form
constexpr uint32_t kPutRejectLimiter = 2u;       // an image names a limiter the engine lacks

}  // namespace rl
