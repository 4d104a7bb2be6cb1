// rl_hot_thresh.hpp — the hot chains' thresholds and searches: where a key's state denies
// (hot_t0, hot_pred_k), the closed-form guesses (hot_tk_guess), the exact wave-wide search
// (wave_first_true), and the wave-uniform re-declarations (uni). Included by rl_hot.hpp.
#pragma once
#include "rl_region.hpp"

#pragma clang fp contract(off)

namespace rl {

// Start of the range on which the thresholds (hot_pred_k) are monotone and valid.
template <int ALGO>
__device__ inline int64_t hot_t0(int64_t lo, int64_t hi, uint64_t a, uint64_t b, uint64_t c) {
    if constexpr (ALGO == kAlgoTB) {
        if (!(c & 1u)) return lo;                               // absent: full at every t
        if (!(__longlong_as_double((long long)a) >= 0.0)) return hi + 1;
        return (int64_t)b > lo ? (int64_t)b : lo;               // t >= last: balance >= 0
    } else {
        const SW2 s = sw_unpack(a, b, c);
        if (s.b1_cnt == 0 && s.b0_cnt == 0) return lo;
        return s.b1_start > lo ? s.b1_start : lo;
    }
}

// First t in [s, hi] with pred(t) for a predicate monotone (false..true) on [s, hi];
// hi + 1 if none. One wave: an exponential bracket (64 probes in one instruction), then
// 64-ary narrowing. Arguments are wave-uniform.
template <class P>
__device__ inline int64_t wave_first_true(int64_t s, int64_t hi, uint32_t lane, P pred) {
    if (s > hi) return hi + 1;
    int64_t t = lane == 0 ? s : (lane < 63 ? s + ((int64_t)1 << (lane - 1)) : hi);
    if (t > hi) t = hi;
    const uint64_t m = __ballot(pred(t));
    if (m == 0) return hi + 1;
    const uint32_t k = (uint32_t)__builtin_ctzll(m);
    if (k == 0) return s;
    int64_t lo = __shfl(t, (int)k - 1, 64) + 1;                 // pred(t_{k-1}) false
    int64_t h = __shfl(t, (int)k, 64);                          // pred(t_k) true
    while (h > lo) {
        const int64_t step = (h - lo + 64) / 64;
        int64_t u = lo + ((int64_t)lane + 1) * step - 1;
        if (u > h) u = h;
        const uint64_t mm = __ballot(pred(u));
        if (mm == 0) return h;                                  // (monotone: not reached)
        const uint32_t kk = (uint32_t)__builtin_ctzll(mm);
        const int64_t uk = __shfl(u, (int)kk, 64);
        const int64_t ukm = __shfl(u, kk ? (int)kk - 1 : 0, 64);
        lo = kk ? ukm + 1 : lo;
        h = uk;
    }
    return lo;
}

// For a fixed state and t >= hot_t0, an acquire of k permits at t is allowed iff t >= T_k,
// the first t with (TB) balance >= k or (SW) estimate <= max - k: the predicate below is
// monotone in t (nested in k).
template <int ALGO>
__device__ inline bool hot_pred_k(const DevLimiter& L, int64_t t, uint64_t a, uint64_t b, uint64_t c,
                                  int64_t k) {
    if constexpr (ALGO == kAlgoTB) {
        return tb_refill(L, t, a, b, c) >= (double)k;
    } else {
        const SW2 s = sw_unpack(a, b, c);
        return sw_estimate(s, sw_geo(t, L), t, L.window_ms) + k <= L.max_permits;
    }
}

// A starting point for T_k from the closed forms (its users check it exactly with
// hot_pred_k: KeyChain::t1_of, KeyChain::thr_build).
template <int ALGO>
__device__ inline int64_t hot_tk_guess(const DevLimiter& L, int64_t s, uint64_t a, uint64_t b,
                                       uint64_t c, int64_t k) {
    if constexpr (ALGO == kAlgoTB) {
        if (!(c & 1u)) return s;                                // absent: full at every t
        const double tok0 = __longlong_as_double((long long)a);
        const int64_t last = (int64_t)b;
        if (!(tok0 < (double)k) || !(L.rate_per_ms > 0.0)) return s;
        const double te = (double)last + ceil(((double)k - tok0) * L.inv_rate);
        const int64_t g = te < 4.0e18 ? (int64_t)te : INT64_MAX / 4;
        const int64_t full = last + L.ttl_ms + 1;               // expired: full again
        return g < full ? g : full;
    } else {
        const int64_t m = L.max_permits - k + 1;                // allowed iff estimate < m
        const int64_t w = L.window_ms;
        const SW2 st = sw_unpack(a, b, c);
        const SWGeo g0 = sw_geo(s, L);
        const int64_t C = sw_get(st, g0.curr_start, s, w);
        const int64_t P = sw_get(st, g0.prev_start, s, w);
        const int64_t wend = g0.curr_start + w;                 // next window: a new geometry
        if (m <= 0) return s;
        if (C < m) {
            if (P == 0) return s;
            // estimate = P * pw + C < m  <=>  now % w > w (1 - (m - C) / P)
            const double rr = (double)w * (1.0 - (double)(m - C) * __builtin_amdgcn_rcp((double)P));
            int64_t g = g0.curr_start + (int64_t)floor(rr) + 1;
            int64_t lastp = INT64_MAX / 4;                      // previous bucket's TTL lapse
            if (st.b1_start == g0.prev_start) lastp = st.b1_start + st.b1_off;
            else if (st.b1_start == g0.curr_start) lastp = g0.prev_start + st.b0_off;
            if (g > lastp + w + 1) g = lastp + w + 1;
            if (g < wend) return g > s ? g : s;
        }
        // not in this window: in the next one the current bucket (C) is the previous one,
        // weighted by pw, until its TTL lapses (last INCR + w)
        if (C < m) return wend;
        const int64_t lastc = st.b1_start == g0.curr_start ? st.b1_start + st.b1_off : wend;
        const double rr = (double)w * (1.0 - (double)m * __builtin_amdgcn_rcp((double)C));
        int64_t g = wend + (int64_t)floor(rr) + 1;
        if (g > lastc + w + 1) g = lastc + w + 1;
        return g;
    }
}

// prev * pw of the sliding-window estimate at `now` (:170-174, rounded as Java rounds) for
// the key state (a, b, c), off the hot chains' fast paths: a call, so that the compiler cannot
// hoist the window geometry and its fp64 division into them (inlined, they were computed for
// every request of every detailed chunk, used or not).
__device__ __attribute__((noinline)) double sw_prev_weighted(int64_t now, uint64_t a, uint64_t b,
                                                             uint64_t c, int64_t w, double inv_w) {
    DevLimiter L{};
    L.window_ms = w;
    L.inv_window = inv_w;
    const SWGeo g = sw_geo(now, L);
    return (double)sw_get(sw_unpack(a, b, c), g.prev_start, now, w) * g.prev_weight;
}

// Wave-uniform values made visibly so (v_readfirstlane into SGPRs): the chains' control flow
// on them then compiles to scalar branches instead of exec-mask regions around 64-bit VALU
// compares, which a lone wave pays for at every step.
__device__ inline uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ inline int32_t uni(int32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ inline uint64_t uni(uint64_t x) {
    return ((uint64_t)uni((uint32_t)(x >> 32)) << 32) | (uint64_t)uni((uint32_t)x);
}
__device__ inline int64_t uni(int64_t x) { return (int64_t)uni((uint64_t)x); }
__device__ inline double uni(double x) {
    return __longlong_as_double((long long)uni((uint64_t)__double_as_longlong(x)));
}
__device__ inline HotInfo uni(const HotInfo& f) {
    HotInfo u;
    u.tag = uni(f.tag); u.bin = uni(f.bin); u.start = uni(f.start); u.end = uni(f.end);
    u.n_chunks = uni(f.n_chunks); u.chunk_base = uni(f.chunk_base); u.ok = uni(f.ok);
    u.n_groups = uni(f.n_groups); u.group_base = uni(f.group_base); u.tag2 = uni(f.tag2);
    return u;
}
__device__ inline DevLimiter uni(const DevLimiter& l) {
    DevLimiter u;
    u.algo = uni(l.algo); u.region_bits = uni(l.region_bits); u.region_base = uni(l.region_base);
    u.lflags = uni(l.lflags); u.max_permits = uni(l.max_permits); u.window_ms = uni(l.window_ms);
    u.ttl_ms = uni(l.ttl_ms); u.rate_per_ms = uni(l.rate_per_ms); u.capacity = uni(l.capacity);
    u.table = uni(l.table); u.inv_window = uni(l.inv_window); u.cache_table = uni(l.cache_table);
    u.cache_ttl_ms = uni(l.cache_ttl_ms); u.inv_rate = uni(l.inv_rate);
    return u;
}

}  // namespace rl
