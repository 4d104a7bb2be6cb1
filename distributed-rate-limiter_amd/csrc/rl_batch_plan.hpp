// rl_batch_plan.hpp — the host arithmetic of one batch (run_batch_device, rl_engine_batch.cpp):
// partition tiles, the digit split of a two-pass partition, hot-region routing, pass-0 segments
// and the word counts of the scratch that depends on them. No HIP call, so it is tested on the
// CPU against brute force (tests/cpp/test_batch_plan.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/rl_engine.h"
#include "rl_launch.hpp"

namespace rl {

inline int ceil_log2(uint64_t x) {
    int b = 0;
    while ((1ULL << b) < x) ++b;
    return b;
}

// The rl_tune values a plan reads.
struct BatchTune {
    uint32_t tile_items = 0;        // partition tile rounds (0: auto)
    uint32_t segments = 1;          // two-pass batches: pass-0 output segments
    uint32_t group_bits = 12;       // two-pass batches: pass-0 high-digit bits
    uint32_t hot_threshold = 16384; // records per region for the hot path; 0 disables
    bool hot_thr_auto = true;       // max(hot_threshold, n / 4096) per batch
    bool route = true;              // hot-region routing in pass 0
    uint32_t up_per_cu = 0;         // upsweep workgroups per CU (0: default)
};

struct BatchPlan {
    uint32_t titems;        // per-thread items of a partition tile
    uint32_t nt;            // partition tiles (titems * kTileThreads requests each)
    uint32_t nt_un;         // unpermute tiles (kTile requests each)
    int bitsP;              // bits of a region id
    int passes;             // 1, or 2: pass 0 by the high dh bits, then k_group inside each bin
    int dh, s0;             // the split: 2^dh pass-0 bins of 2^s0 consecutive regions
    bool hot;               // the hot path is on
    bool route;             // pass 0 gets kRouteBins dense bins beyond the 2^dh high-digit ones
    uint32_t nb0;           // pass-0 bins
    int digit_bits;         // bits of a pass-0 digit
    uint32_t seg_tiles;     // segmented pass-0 output: n_segs runs of seg_tiles tiles
    uint32_t n_segs;
    uint32_t hot_thr;       // records per region for the hot path
    uint32_t up_per_cu;
    size_t counts_words;    // [bin][tile] counts
    size_t seg_words;       // seg_adj, seg_start, seg_cnt (0: not segmented)
    uint32_t tile_recs;     // k_group: records per tile, tiles the scratch holds (0: one pass)
    uint32_t max_tiles;
    size_t gtile_words;     // k_group: tile_base, tile_bin, per-tile counts, tile_beg / tile_end
};

// The plan of a batch of n > 0 requests over n_regions regions (one partition bin per region).
// RL_E_LIMITERS: more regions than two digits address.
inline int plan_batch(const BatchTune& t, size_t n, uint32_t n_regions, BatchPlan* out) {
    BatchPlan p{};
    // partition tiles of 128K requests for large batches (half the [bin][tile] counts to write
    // and scan: sw_zipf's 2^28-request batches, scan0 0.16 -> 0.06 ms, upsweep0 0.89 -> 0.75 ms),
    // 64K below (tb_uniform's 2^26 needs the 1024 tiles to keep every CU busy; the unpermute keeps
    // 64K tiles)
    p.titems = t.tile_items ? t.tile_items
                            : (n >= ((size_t)3 << 26) ? 2u * kTileItems : (uint32_t)kTileItems);
    const size_t tile_n = (size_t)p.titems * kTileThreads;
    p.nt = (uint32_t)((n + tile_n - 1) / tile_n);
    p.nt_un = (uint32_t)((n + kTile - 1) / kTile);
    p.bitsP = std::max(1, ceil_log2(n_regions));
    p.passes = p.bitsP <= kMaxDigitBits ? 1 : 2;
    if (p.bitsP > 2 * kMaxDigitBits) return RL_E_LIMITERS;
    // Two passes: pass 0 partitions by the high dh bits of the region id (2^dh bins of 2^s0
    // consecutive regions), then rl_group.hip groups each bin by region locally
    p.dh = p.passes == 1 ? p.bitsP
                         : std::max(p.bitsP - kMaxDigitBits, std::min<int>((int)t.group_bits, kMaxDigitBits));
    p.s0 = p.bitsP - p.dh;
    // hot-region routing: pass 0 gets kRouteBins dense bins beyond the 2^dh high-digit ones. The
    // hot path is gated per limiter: regions of a limiter with the local cache are never
    // listed hot (k_hot_select), so they are never routed either; the other limiters keep it.
    p.hot = t.hot_threshold > 0;
    p.route = p.hot && t.route && p.passes == 2 && (1u << p.dh) + kRouteBins <= (1u << kMaxDigitBits);
    p.nb0 = p.route ? (1u << p.dh) + kRouteBins : 1u << p.dh;
    p.digit_bits = p.route ? ceil_log2(p.nb0) : p.dh;
    // segmented pass-0 output (two passes): n_segs runs of seg_tiles tiles
    p.seg_tiles = p.passes == 2 && t.segments > 1 ? (p.nt + t.segments - 1) / t.segments : p.nt;
    p.n_segs = (p.nt + p.seg_tiles - 1) / p.seg_tiles;
    // records per region for the hot path: scaled with the batch by default (measured per
    // config: sw_zipf best at 65536 for 2^28 requests, zipf_1b at 32768 for 2^27)
    p.hot_thr = t.hot_thr_auto ? std::max<uint32_t>(t.hot_threshold, (uint32_t)(n >> 12)) : t.hot_threshold;
    // (128K-request tiles: one upsweep tile per workgroup, 8 per CU: upsweep0 0.76 -> 0.73 ms on
    // sw_zipf over 6 runs)
    p.up_per_cu = t.up_per_cu ? t.up_per_cu : (p.titems > (uint32_t)kTileItems ? 8u : 0u);
    p.counts_words = (size_t)p.nb0 * p.nt;
    if (p.n_segs > 1) p.seg_words = (size_t)3 * p.nb0 * p.n_segs;
    if (p.passes == 2) {
        // every (bin, segment) run ends in at most one partly filled tile
        const uint32_t n_bins0 = 1u << p.dh;
        p.tile_recs = group_tile_recs((uint32_t)p.s0);
        p.max_tiles = (uint32_t)((n + p.tile_recs - 1) / p.tile_recs) + n_bins0 * p.n_segs;
        p.gtile_words = (size_t)n_bins0 + 1 + (size_t)p.max_tiles * (1 + ((size_t)1 << p.s0)) +
                        (p.n_segs > 1 ? (size_t)2 * p.max_tiles : 0);
    }
    *out = p;
    return RL_OK;
}

}  // namespace rl
