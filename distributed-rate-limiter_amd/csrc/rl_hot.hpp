// rl_hot.hpp — 4b. hot regions: dominant-key chains, their summaries and fills (templates;
// rl_hot.hip holds the untemplated kernels and the launchers, rl_rt_*.hip the instantiations).
// The parts, each a header of its own:
//   rl_hot_words.hpp   the summary / verdict word format (the interface between the phases)
//   rl_hot_thresh.hpp  thresholds and searches (hot_t0, hot_pred_k, hot_tk_guess, uni)
//   rl_hot_summ.hpp    k_hot_prep, k_hot_summ
//   rl_hot_detail.hpp  the chain's and a key's state, one chunk record by record (detail)
//   rl_hot_walk.hpp    the allow walk (walk)
//   rl_hot_chain.hpp   hot_chain, k_hot_chains
//   rl_hot_fill.hpp    k_hot_fill, walk_fill_key
#pragma once
#include "rl_region.hpp"

#pragma clang fp contract(off)

namespace rl {

// ------------------------------------------------------------------ 4b. hot regions
// A region far above the average share (a hot Zipf key: at s = 1.1 over 100M keys the
// top key draws 11 % of all requests) would serialise one wave, and one CU's memory
// bandwidth, for the whole batch. Its dominant key (the HOT key) gets a fast path:
//  * a deny never changes state (SlidingWindowRateLimiter.java:104-111,
//    TokenBucketRateLimiter.java:61-67);
//  * for a fixed state the SW estimate (:158-180) is non-increasing in `now` for `now`
//    at or after the newest bucket, and the TB balance (Lua :46-58) is non-decreasing.
// So one threshold pair [T0, T1) per state holds exactly the times at which a request is
// denied with remaining 0 (SW: est >= max; TB: 0 <= balance < 1), whatever its permits.
// Inside an undecided chunk the further thresholds T_2.. decide the other denials by
// integer compares (hot_pred_k); the allowed request, a peek or a reset runs the
// exact step alone, and after each state change the thresholds are found again by an
// exact search that evaluates the very same arithmetic (tb_refill, sw_estimate) at 64
// times per wave instruction. Three phases:
//  A  k_hot_summ   (all CUs)  per 64 records: time range of the hot key's plain acquires,
//                              count of records that need the exact path;
//  B  k_hot_chains (one wave per hot region, beside k_regions) goes down the summaries with
//                              [T0, T1), decides whole chunks unread, processes the rest
//                              record by record (other keys through wave_apply);
//  C  k_hot_fill   (all CUs)  writes the results of the decided chunks.

// A key the walk pays for, from its expected allows e (an upper estimate: TB a full bucket plus
// the refill over the batch's span; SW the limit per window over the windows the span
// touches): at least walk_min of them (kWalkMinAllows), so that the chain is long, and at most
// 2.5 per 64-record chunk: denser keys allow several times per chunk, which the chunk-by-chunk
// path decides at one detail per chunk.
__device__ inline bool walk_dense(const HotInfo& f, const DevLimiter& L, int64_t lo, int64_t hi,
                                  uint32_t walk_min) {
    const double span = (double)(hi - lo + 1);
    const double e = L.algo == kAlgoTB ? L.capacity + L.rate_per_ms * span
                                       : (double)L.max_permits * (span / (double)L.window_ms + 2.0);
    return e >= (double)walk_min && 2.0 * e <= 5.0 * (double)f.n_chunks;
}

// Allow walks (rl_hot_walk.hpp): is region i's key table built in this batch (slot 2 i + key)?
__device__ inline bool walk_table_on(const RegionArgs& a, uint32_t i, const HotInfo& f,
                                     const DevLimiter& L, int64_t lo, int64_t hi) {
    return a.walk_tab && i < walk_regions(lo, hi) && f.end - f.start < (1u << 31) &&
           walk_dense(f, L, lo, hi, a.walk_min);
}

}  // namespace rl

#include "rl_hot_summ.hpp"
#include "rl_hot_chain.hpp"
#include "rl_hot_fill.hpp"

namespace rl {

// The chain launch on the side stream hs: single-wave workgroups looping over the hot list,
// or (chain_split) one two-wave workgroup per possible hot region.
template <class Codec, class Res>
hipError_t hot_chains_t(const RegionArgs& a, hipStream_t hs) {
    if (a.chain_split) {
        const dim3 g(kHotMax);
        if (a.tok) hipLaunchKernelGGL((k_hot_chains<Codec, Res, true, true>), g, dim3(128), 0, hs, a);
        else hipLaunchKernelGGL((k_hot_chains<Codec, Res, false, true>), g, dim3(128), 0, hs, a);
        return hipGetLastError();
    }
    const dim3 g(a.chain_grid ? min(a.chain_grid, kHotMax) : kHotMax);
    if (a.tok) hipLaunchKernelGGL((k_hot_chains<Codec, Res, true, false>), g, dim3(64), 0, hs, a);
    else hipLaunchKernelGGL((k_hot_chains<Codec, Res, false, false>), g, dim3(64), 0, hs, a);
    return hipGetLastError();
}
template <class Codec, class Res>
hipError_t hot_fill_t(const RegionArgs& a, hipStream_t s) {
    const dim3 gp(persistent_grid(1u << 30, 4));
    if (a.tok) hipLaunchKernelGGL((k_hot_fill<Codec, Res, true, false>), gp, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_hot_fill<Codec, Res, false, false>), gp, dim3(256), 0, s, a);
    if (a.walk_tab) {                                 // (allow walks on: their verdicts)
        if (a.tok) hipLaunchKernelGGL((k_hot_fill<Codec, Res, true, true>), gp, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_hot_fill<Codec, Res, false, true>), gp, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace rl
