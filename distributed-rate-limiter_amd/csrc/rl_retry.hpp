// rl_retry.hpp — what the per-key query kernels share: retry-after (rl_retry.hip) and the quota
// lookup (rl_quota.hip). A wave answers 64 queries, lane i owning query i; it looks the 64 keys
// up sixteen at a time with the quad probe of rl_table.hpp (wave_lookup), and every lane then
// searches on its own key's slot words (retry_search).
//
// Both algorithms are monotone for a fixed state from the key's newest write on (the sliding
// window's estimate never rises, the token balance never falls: DESIGN.md §4), so the answer
// is the one t with P(t) and not P(t - 1). The search takes a closed-form guess, checks it and
// its neighbours with the exact predicate (tb_step / sw_step_g / sw_step_cache of
// rl_device.hpp, the same code the region stage runs), and bisects with that predicate when
// the guess is off by more than two. Guesses use any arithmetic; every returned value is one
// the exact predicate confirmed at t and refuted at t - 1.
#pragma once
#include "rl_table.hpp"

#pragma clang fp contract(off)

namespace rl {

__device__ inline int64_t imax(int64_t x, int64_t y) { return x > y ? x : y; }

// What getAvailablePermits reads at millisecond t on state (a, b, c): RL_OP_PEEK's remaining.
// The local cache does not count: the reference's getAvailablePermits reads the counters only.
__device__ inline int64_t peek_remaining(const DevLimiter& L, int64_t t, uint64_t a, uint64_t b, uint64_t c) {
    if (L.algo == kAlgoTB) return tb_step(L, kOpPeek, 1, t, a, b, c).remaining;
    return sw_step_g(L, kOpPeek, 1, t, sw_geo(t, L), a, b, c).remaining;
}

// P(t): an acquire of p at millisecond t is allowed on state (a, b, c, x), not applied. With
// `full`, p and x are not looked at and P(t) is "the whole quota is available at t": the peek
// reads maxPermits. That is an acquire of maxPermits with the cache word ignored (SW:
// est + max > max iff est >= 1; TB: min(cap, ..) >= cap iff (long)tokens == cap; DESIGN.md §4
// "Quota queries"), stated on the peek so that a token bucket's maxPermits beyond int32 needs no cast.
__device__ inline bool retry_pred(const DevLimiter& L, bool full, int32_t p, int64_t t, uint64_t a,
                                  uint64_t b, uint64_t c, uint64_t x) {
    if (full) return peek_remaining(L, t, a, b, c) == L.max_permits;
    if (L.algo == kAlgoTB) return tb_step(L, kOpAcquire, p, t, a, b, c).allowed;
    const SWGeo g = sw_geo(t, L);
    if (L.cache_ttl_ms > 0) {
        bool hit;
        return sw_step_cache(L, kOpAcquire, p, t, g, a, b, c, x, hit).allowed;
    }
    return sw_step_g(L, kOpAcquire, p, t, g, a, b, c).allowed;
}

// Earliest t in [max(W, lo), W + w) with prev * (1 - (t - W) / w) + curr < room (the estimate
// of :170-174 at most max - p), or -1. A first guess: rounded like nothing in particular.
__device__ inline int64_t sw_guess_window(int64_t W, int64_t lo, double prev, double curr, double room,
                                          int64_t w) {
    const double need = room - curr;
    if (!(need > 0.0)) return -1;
    int64_t t = W;
    if (prev > 0.0 && !(prev < need)) {
        const double rr = (double)w * (1.0 - need / prev);       // in [0, w)
        t = W + (int64_t)rr + 1;
    }
    if (t < lo) t = lo;
    return t < W + w ? t : -1;
}

// The wait of one query whose key has a slot. P is false before t0 = max(now, the cache
// word, the key's newest INCR) only through the cache word, and true at `hi` (SW: two windows
// after the newest bucket's start nothing is in view; TB: the hash has expired and reads full).
// `full` (retry_pred): the wait for the whole quota, p = maxPermits with the cache word ignored.
__device__ inline int64_t retry_search(const DevLimiter& L, bool full, int32_t p, int64_t now, uint64_t a,
                                       uint64_t b, uint64_t c, uint64_t x, bool& bisected) {
    const int64_t w = L.window_ms;
    bisected = false;
    int64_t t0 = now, hi;
    const SW2 s = sw_unpack(a, b, c);
    if (L.algo == kAlgoTB) {
        hi = (int64_t)b + L.ttl_ms + 1;
    } else {
        // a query before the key's newest INCR (time regression, outside the batch calls' own
        // contract) is searched from that INCR's time; the wait still counts from now
        if (s.b1_cnt != 0) t0 = imax(t0, s.b1_start + s.b1_off);
        else if (s.b0_cnt != 0) t0 = imax(t0, s.b1_start - w + s.b0_off);
        if (!full && L.cache_ttl_ms > 0) t0 = imax(t0, (int64_t)x);
        hi = s.b1_start + 2 * w;
    }
    if (retry_pred(L, full, p, t0, a, b, c, x)) return t0 - now;
    // ---- the guess
    const double pd = full ? (double)L.max_permits : (double)p;
    int64_t g;
    if (L.algo == kAlgoTB) {
        const int64_t last = (int64_t)b;
        double d = __builtin_ceil((pd - __longlong_as_double((long long)a)) * L.inv_rate);
        const double cap = (double)(L.ttl_ms + 1);
        if (!(d < cap)) d = cap;                       // expiry at last + 2w + 1 comes first
        if (!(d > 0.0)) d = 0.0;
        g = last + (int64_t)d;
    } else {
        const int64_t W1 = sw_geo(t0, L).curr_start;
        // the buckets of W1 (count n1, PEXPIRE deadline E1) and W1 - w (n0, E0)
        double n1 = 0.0, n0 = 0.0;
        int64_t E1 = W1 + w - 1, E0 = W1 - 1;
        if (s.b1_start == W1) {
            if (s.b1_cnt) { n1 = (double)s.b1_cnt; E1 = s.b1_start + s.b1_off + w; }
            if (s.b0_cnt) { n0 = (double)s.b0_cnt; E0 = s.b1_start + s.b0_off; }
        } else if (s.b1_start == W1 - w) {
            if (s.b1_cnt) { n0 = (double)s.b1_cnt; E0 = s.b1_start + s.b1_off + w; }
        }
        const double room = full ? 1.0 : (double)(L.max_permits - (int64_t)p + 1);
        const int64_t lo = t0 + 1, W2 = W1 + w;
        g = -1;
        int64_t t = sw_guess_window(W1, lo, n0, n1, room, w);     // W1, previous bucket alive
        if (t >= 0 && t <= E0) g = t;
        if (g < 0 && n1 < room) {                                 // W1, previous bucket expired
            t = imax(imax(E0 + 1, lo), W1);
            if (t < W2) g = t;
        }
        if (g < 0) {                                              // W2: W1's bucket is the previous
            t = sw_guess_window(W2, imax(lo, W2), n1, 0.0, room, w);
            if (t >= 0 && t <= E1) g = t;
            else g = imax(E1 + 1, W2);                             // expired (or W2 + w: nothing in view)
        }
    }
    if (g > hi) g = hi;
    if (g < t0 + 1) g = t0 + 1;
    // ---- the guess and two neighbours either way, by the exact predicate
    int64_t lo_f = t0;                  // P false (evaluated)
    int64_t hi_t = hi;                  // P true once hi_known
    bool hi_known = false;
    int64_t t = g;
    if (retry_pred(L, full, p, t, a, b, c, x)) {
        for (int k = 0;; ++k) {
            if (t - 1 == t0 || !retry_pred(L, full, p, t - 1, a, b, c, x)) return t - now;
            --t;
            if (k == 2) break;
        }
        hi_t = t; hi_known = true;
    } else {
        lo_f = t;
        for (int k = 0; k < 2 && t < hi; ++k) {
            ++t;
            if (retry_pred(L, full, p, t, a, b, c, x)) return t - now;
            lo_f = t;
        }
    }
    // ---- bisection on (lo_f: false, hi_t: true)
    bisected = true;
    if (!hi_known && !retry_pred(L, full, p, hi_t, a, b, c, x)) return kRetryNever;   // (excluded: see above)
    while (hi_t - lo_f > 1) {
        const int64_t mid = lo_f + (hi_t - lo_f) / 2;
        if (retry_pred(L, full, p, mid, a, b, c, x)) hi_t = mid;
        else lo_f = mid;
    }
    return hi_t - now;
}

// ------------------------------------------------------------------ the 64-query wave lookup
constexpr int kRetryThreads = 256;
constexpr int kRetryPerQuad = 4;                          // lookup steps of a wave: 16 keys each
constexpr int kRetryWaveQueries = 16 * kRetryPerQuad;     // per wave
constexpr int kRetryBlockQueries = (kRetryThreads / 64) * kRetryWaveQueries;
constexpr uint32_t kLimWords = sizeof(DevLimiter) / sizeof(uint64_t);
static_assert(sizeof(DevLimiter) % sizeof(uint64_t) == 0, "DevLimiter is copied to LDS in 8-B words");

enum : uint32_t { kZero = 0, kInvalid = 1, kNever = 2, kProbe = 3 };   // a query after its decode

// The limiter table into the workgroup's LDS (kLimWords words per limiter), by all its threads;
// the caller's __syncthreads comes before the first use.
__device__ inline void limiters_to_lds(uint64_t* s_limw, const DevLimiter* lims, uint32_t n_lim) {
    const uint64_t* src = (const uint64_t*)lims;
    for (uint32_t w = threadIdx.x; w < n_lim * kLimWords; w += kRetryThreads) s_limw[w] = src[w];
}

// a[k] = a[k + 1]: the per-query loop below always works on element 0 and shifts the rest
// down, so the arrays stay in registers (constant indices) and the loop body exists once
template <class T, int N>
__device__ inline void shift_down(T (&a)[N]) {
#pragma unroll
    for (int k = 0; k + 1 < N; ++k) a[k] = a[k + 1];
}

// The slot words of this lane's own key ({a, b, c}, the cache word) and whether it has a slot.
struct KeyState { uint64_t a, b, c, x; bool have; };

// The wave looks its 64 keys up sixteen at a time, four lanes per key: in step j quad k serves
// the query of lane 16 j + k. Tag and limiter go to the quad, and the slot it finds goes back
// to its owner, by lane permutes. `h` is the lane's mixed key and `st` its limiter << 2 | code;
// only a query with code kProbe touches the table. The home buckets of all four steps load
// together; the limiter table is read from LDS (s_lims). Called by every lane of the wave.
// `probed` (measurement builds of k_retry_after, else null) counts the buckets probed.
__device__ inline KeyState wave_lookup(const DevLimiter* s_lims, int shard_bits, uint64_t h, uint32_t st,
                                       uint32_t lane, unsigned long long* probed) {
    constexpr int Q = kRetryPerQuad;
    const uint32_t sub = lane & 3;
    // ---- the home buckets of all four steps, loaded together
    uint32_t stq[Q];                     // the served query's limiter << 2 | code
    uint64_t hq[Q];
    QuadSlot vq[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        const int owner = 16 * j + (int)(lane >> 2);
        hq[j] = (uint64_t)shfl64((int64_t)h, owner);
        stq[j] = (uint32_t)__shfl((int)st, owner, 64);
        vq[j] = QuadSlot{{0, 0}, {0, 0}, 0};
        if ((stq[j] & 3u) == kProbe)
            vq[j] = quad_load(table_region(s_lims[stq[j] >> 2], hq[j], shard_bits), quad_pos(hq[j], 0, sub));
    }
    // ---- per step (one copy of this code: it works on element 0 and shifts the others down):
    // the keys' slots, handed to the lanes that own the queries
    KeyState ks{0, 0, 0, 0, false};
#pragma unroll 1
    for (int j = 0; j < Q; ++j) {
        bool op = (stq[0] & 3u) == kProbe;         // still probing
        const uint64_t hj = hq[0];
        QuadSlot v = vq[0];
        bool mine = false;                         // this lane holds the key's slot
        // the quad probe (rl_table.hpp) from the preloaded home bucket on
        for (uint32_t m = 0;; ++m) {               // (wave-uniform trip count; nearly always one)
#ifdef RL_RETRY_COUNT
            if (op && probed && sub == 0) atomicAdd(probed, 1ULL);
#endif
            quad_resolve(op, v, hj, lane, mine);
            if (m + 1 == kProbeBuckets) op = false;            // a full region without the key: absent
            if (!__any(op)) break;
            if (op)                                // the next bucket
                v = quad_load(table_region(s_lims[stq[0] >> 2], hj, shard_bits), quad_pos(hj, m + 1, sub));
        }
        // lane 16 j + k takes the slot that quad k found (at most one lane of a quad has one)
        const uint64_t mm = __ballot(mine);
        const uint32_t nib = (uint32_t)(mm >> (4 * (lane & 15u))) & 0xFu;    // quad (lane & 15)'s lanes
        const int from = (int)(4 * (lane & 15u)) + (nib ? __builtin_ctz(nib) : 0);
        const uint64_t ta = (uint64_t)shfl64((int64_t)v.lo.y, from);
        const uint64_t tb = (uint64_t)shfl64((int64_t)v.hi.x, from);
        const uint64_t tc = (uint64_t)shfl64((int64_t)v.hi.y, from);
        uint64_t tx = 0;
        if (__any(mine && v.x != 0)) tx = (uint64_t)shfl64((int64_t)v.x, from);   // (cache-on limiters only)
        if ((int)(lane >> 4) == j && nib != 0) ks = KeyState{ta, tb, tc, tx, true};
        shift_down(stq); shift_down(hq); shift_down(vq);
    }
    (void)probed;
    return ks;
}

}  // namespace rl
