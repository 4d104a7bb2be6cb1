// rl_retry.hip — batched retry-after queries: for (limiter, key, permits, now) the first
// millisecond t >= now at which tryAcquire(key, permits) would be allowed on the key's state
// as it stands, without applying it (rl_retry_after, include/rl_engine.h).
//
// A read-only gather: no partition, no region image, no atomics, no table write. Four lanes
// look one key up (16 keys per wave at a time) with the quad probe of rl_table.hpp. A wave takes
// 64 queries, so it does four such steps with their home-bucket loads in flight together; the
// slots then go to the lanes that own the queries, and every lane searches for its own answer
// and stores it. The limiter table sits in LDS (the only LDS use).
//
// Both algorithms are monotone for a fixed state from the key's newest write on (the sliding
// window's estimate never rises, the token balance never falls: DESIGN.md §4), so the answer
// is the one t with P(t) and not P(t - 1). The search takes a closed-form guess, checks it and
// its neighbours with the exact predicate (tb_step / sw_step_g / sw_step_cache of
// rl_device.hpp, the same code the region stage runs), and bisects with that predicate when
// the guess is off by more than two. Guesses use any arithmetic; every returned value is one
// the exact predicate confirmed at t and refuted at t - 1.
#include "rl_table.hpp"

#pragma clang fp contract(off)

namespace rl {

__device__ inline int64_t imax(int64_t x, int64_t y) { return x > y ? x : y; }

// P(t): an acquire of p at millisecond t is allowed on state (a, b, c, x), not applied.
__device__ inline bool retry_pred(const DevLimiter& L, int32_t p, int64_t t, uint64_t a, uint64_t b,
                                  uint64_t c, uint64_t x) {
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
__device__ inline int64_t retry_search(const DevLimiter& L, int32_t p, int64_t now, uint64_t a,
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
        if (L.cache_ttl_ms > 0) t0 = imax(t0, (int64_t)x);
        hi = s.b1_start + 2 * w;
    }
    if (retry_pred(L, p, t0, a, b, c, x)) return t0 - now;
    // ---- the guess
    int64_t g;
    if (L.algo == kAlgoTB) {
        const int64_t last = (int64_t)b;
        double d = __builtin_ceil(((double)p - __longlong_as_double((long long)a)) * L.inv_rate);
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
        const double room = (double)(L.max_permits - (int64_t)p + 1);
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
    if (retry_pred(L, p, t, a, b, c, x)) {
        for (int k = 0;; ++k) {
            if (t - 1 == t0 || !retry_pred(L, p, t - 1, a, b, c, x)) return t - now;
            --t;
            if (k == 2) break;
        }
        hi_t = t; hi_known = true;
    } else {
        lo_f = t;
        for (int k = 0; k < 2 && t < hi; ++k) {
            ++t;
            if (retry_pred(L, p, t, a, b, c, x)) return t - now;
            lo_f = t;
        }
    }
    // ---- bisection on (lo_f: false, hi_t: true)
    bisected = true;
    if (!hi_known && !retry_pred(L, p, hi_t, a, b, c, x)) return kRetryNever;   // (excluded: see above)
    while (hi_t - lo_f > 1) {
        const int64_t mid = lo_f + (hi_t - lo_f) / 2;
        if (retry_pred(L, p, mid, a, b, c, x)) hi_t = mid;
        else lo_f = mid;
    }
    return hi_t - now;
}

constexpr int kRetryThreads = 256;
constexpr int kRetryPerQuad = 4;                          // lookup steps of a wave: 16 keys each
constexpr int kRetryWaveQueries = 16 * kRetryPerQuad;     // per wave
constexpr int kRetryBlockQueries = (kRetryThreads / 64) * kRetryWaveQueries;
constexpr uint32_t kLimWords = sizeof(DevLimiter) / sizeof(uint64_t);
static_assert(sizeof(DevLimiter) % sizeof(uint64_t) == 0, "DevLimiter is copied to LDS in 8-B words");

enum : uint32_t { kZero = 0, kInvalid = 1, kNever = 2, kProbe = 3 };   // a query after its decode

// a[k] = a[k + 1]: the per-query loop below always works on element 0 and shifts the rest
// down, so the arrays stay in registers (constant indices) and the loop body exists once
template <class T, int N>
__device__ inline void shift_down(T (&a)[N]) {
#pragma unroll
    for (int k = 0; k + 1 < N; ++k) a[k] = a[k + 1];
}

// A wave answers 64 consecutive queries, lane i owning query i: it reads the request and, at
// the end, searches and stores the answer (coalesced, every lane busy in the search). In
// between the wave looks the 64 keys up sixteen at a time, four lanes per key: in step j quad k
// serves the query of lane 16 j + k. Tag and limiter go to the quad, and the slot it finds goes
// back to its owner, by lane permutes. The dependent global loads are two deep (the request
// arrays, then the home buckets of all four steps at once); the limiter table is read from LDS,
// where the workgroup puts it while the request loads are in flight.
__global__ __launch_bounds__(kRetryThreads, 4) void k_retry_after(RetryArgs a) {
    extern __shared__ uint64_t s_limw[];
    const DevLimiter* s_lims = (const DevLimiter*)s_limw;
    constexpr int Q = kRetryPerQuad;
    const uint32_t lane = threadIdx.x & 63, sub = lane & 3;
    const uint32_t q = blockIdx.x * kRetryBlockQueries + threadIdx.x;      // this lane's query
    // ---- the request (a skipped one touches no table)
    uint64_t key = 0;
    int64_t now_ns = 0;
    int32_t p = 0;
    uint32_t lim = 0;
    uint8_t sk = 0;
    if (q < a.n) {
        key = a.key[q];
        now_ns = a.now_ns[q];
        p = a.permits[q];
        if (a.limiter) lim = a.limiter[q];
        if (a.skip) sk = a.skip[q];
    }
    {
        const uint64_t* src = (const uint64_t*)a.lims;
        for (uint32_t w = threadIdx.x; w < a.n_lim * kLimWords; w += kRetryThreads) s_limw[w] = src[w];
    }
    __syncthreads();
    uint32_t code = kZero;
    if (q < a.n && sk == 0) {
        if (lim >= a.n_lim || p <= 0) code = kInvalid;
        else if ((int64_t)p > s_lims[lim].max_permits) code = kNever;   // :110-116; SW est >= 0
        else code = kProbe;
    }
    const uint64_t h = code == kProbe ? mix64(key) : 0;
    const uint32_t st = (code == kProbe ? lim << 2 : 0u) | code;
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
            vq[j] = quad_load(table_region(s_lims[stq[j] >> 2], hq[j], a.shard_bits), quad_pos(hq[j], 0, sub));
    }
    // ---- per step (one copy of this code: it works on element 0 and shifts the others down):
    // the keys' slots, handed to the lanes that own the queries
    uint64_t va = 0, vb = 0, vc = 0, vx = 0;       // this lane's own key's state
    bool have = false;                             // ... which has a slot
#pragma unroll 1
    for (int j = 0; j < Q; ++j) {
        bool op = (stq[0] & 3u) == kProbe;         // still probing
        const uint64_t hj = hq[0];
        QuadSlot v = vq[0];
        bool mine = false;                         // this lane holds the key's slot
        // the quad probe (rl_table.hpp) from the preloaded home bucket on
        for (uint32_t m = 0;; ++m) {               // (wave-uniform trip count; nearly always one)
#ifdef RL_RETRY_COUNT
            if (op && a.dbg && sub == 0) atomicAdd(a.dbg + 2, 1ULL);
#endif
            quad_resolve(op, v, hj, lane, mine);
            if (m + 1 == kProbeBuckets) op = false;            // a full region without the key: absent
            if (!__any(op)) break;
            if (op)                                // the next bucket
                v = quad_load(table_region(s_lims[stq[0] >> 2], hj, a.shard_bits), quad_pos(hj, m + 1, sub));
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
        if ((int)(lane >> 4) == j && nib != 0) { va = ta; vb = tb; vc = tc; vx = tx; have = true; }
        shift_down(stq); shift_down(hq); shift_down(vq);
    }
    // ---- the answer (skipped 0, invalid, never; an absent key grants any p <= max at once: 0)
    int64_t out = code == kInvalid ? kRetryInvalid : code == kNever ? kRetryNever : 0;
    if (code == kProbe && have) {
        bool bis;
        out = retry_search(s_lims[lim], p, floor_div_ms(now_ns), va, vb, vc, vx, bis);
#ifdef RL_RETRY_COUNT
        if (a.dbg) {
            atomicAdd(a.dbg, 1ULL);
            if (bis) atomicAdd(a.dbg + 1, 1ULL);
        }
#endif
    }
    if (q < a.n) a.wait_ms[q] = out;
}

hipError_t launch_retry_after(const RetryArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint32_t grid = (a.n + kRetryBlockQueries - 1) / kRetryBlockQueries;
    const size_t lds = (size_t)(a.n_lim ? a.n_lim : 1) * sizeof(DevLimiter);
    hipLaunchKernelGGL(k_retry_after, dim3(grid), dim3(kRetryThreads), lds, s, a);
    return hipGetLastError();
}

}  // namespace rl
