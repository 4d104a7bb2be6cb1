// rl_small.hip — the small-batch path: one workgroup decides a whole batch of at most
// kSmallMax requests in one launch (k_small_batch), for gfx950. The decisions are the region
// code's (region_body_t, rl_region.hpp): this unit only loads, validates and encodes the
// requests, partitions them by region in LDS (the rule and its addressing: rl_small.hpp), hands
// the touched regions to its waves, folds the batch's control block and writes the results
// back in arrival order.
#include "rl_region.hpp"
#include "rl_small.hpp"

#pragma clang fp contract(off)

namespace rl {

// LDS of the partition (phases 1-2). It is dead once the records are in the scratch, so the
// waves' region tables (phase 3) lie over it.
struct SmallSort {
    uint64_t key[kSmallMax];          // small_sort_key per request
    uint32_t reg[kSmallMax];          // region per sorted position
    uint32_t wcnt[kSmallHeadWaves];   // heads per wave of sorted positions
};
template <class TableT>
union SmallLds {
    SmallSort sort;
    TableT tab[kSmallWaves];
};

template <class T>
__device__ inline T ld_agent(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Hand-overs between the waves (all of one workgroup, so of one CU and one vector L1):
//  (A) the __syncthreads() after the control block's first fields and the LDS limiter table:
//      base_ms and the stats words' zeros (thread 0) before any wave uses them.
//  (B) __syncthreads_or(): every thread's sort key in LDS, and the time range's LDS atomics,
//      before the ranks and before thread 0 publishes the range to the control block.
//  (C) the __syncthreads() after the ranks: reg[] (LDS) before the heads and tails read their
//      neighbours.
//  (D) the __syncthreads() after the head counts: wcnt[] (LDS) before the list slots.
//  (E) the __syncthreads() before phase 3: the records, rstart / rend, the touched list and its
//      length, and the control block's time range and span_overflow, all plain global stores of
//      any wave, before the region waves load them; it also ends every read of the partition's
//      LDS before the region tables overwrite it. A workgroup barrier orders the global stores
//      of a workgroup for its own waves (release / acquire at workgroup scope; the waves share
//      the L1, which these addresses enter only after the stores).
//  (F) the __syncthreads() after phase 3: the packed results, escaped remainders and balances
//      (plain stores of the region waves) before phase 5 gathers them; the statistics and the
//      control block's grow bits, n_esc and internal_err were changed by device-scope atomics,
//      which work in L2, and lines of the control block were loaded into L1 before them: thread 0
//      reads those words back with agent-scope atomic loads (ld_agent), not plain ones.
template <bool CACHE>
__global__ __launch_bounds__(kSmallThreads) void k_small_batch(SmallArgs a) {
    using TableT = typename std::conditional<CACHE, RegionTableX, RegionTable>::type;
    __shared__ SmallLds<TableT> lds;
    __shared__ LimLds L;
    __shared__ unsigned long long s_mn, s_mx;
    __shared__ uint32_t s_tot;
    const uint32_t t = threadIdx.x, lane = t & 63, wid = t >> 6, n = a.n;
    BatchCtl* ctl = a.ra.ctl;
    unsigned long long* stats = a.ra.stats;               // slot 0: the one workgroup's
    load_lim_lds(L, a.ra.lims, a.n_lim);
    const int64_t base = floor_div_ms(a.now_ns[0]) - (1LL << 31);    // as k_upsweep
    if (t == 0) {
        s_mn = ~0ULL;
        s_mx = 0;
        ctl->base_ms = base;
        ctl->n_esc = 0;
        ctl->grow[0] = ctl->grow[1] = ctl->grow[2] = ctl->grow[3] = 0;
        ctl->internal_err = 0;
        for (uint32_t k = 0; k < kStWords; ++k) stats[k] = 0;
    }
    __syncthreads();                                                  // (A)

    // ---- 1. load, validate, encode; the batch's time range
    RecC rec[kSmallPer];
    uint32_t reg[kSmallPer], pos[kSmallPer];
    uint64_t mn = ~0ULL, mx = 0;
    bool over = false;
#pragma unroll
    for (uint32_t k = 0; k < kSmallPer; ++k) {
        const uint32_t i = small_index(t, k);
        rec[k] = RecC{};
        reg[k] = 0;
        pos[k] = 0;
        if (i < n) {
            uint32_t lim = a.limiter ? a.limiter[i] : 0u, op = a.op ? a.op[i] : 0u;
            const int32_t p = a.permits[i];
            const int64_t now_ms = floor_div_ms(a.now_ns[i]);
            const bool invalid = small_invalid(a.n_lim, lim, op, p);
            if (lim >= a.n_lim) lim = 0;                  // decided invalid in limiter 0's region
            if (op > 2u) op = 0;
            const uint64_t h = mix64(a.key[i]);
            rec[k] = CodecC::enc(h, now_ms, base, p, op, lim, invalid);
            reg[k] = region_of(L, h, lim, a.ra.shard_bits);
            if (!invalid) {                               // an invalid request's now is never read
                const int64_t rel = now_ms - base;
                over |= rel < 0 || rel > 0xFFFFFFFFLL;
                const uint64_t ok = ord_key(now_ms);
                mn = ok < mn ? ok : mn;
                mx = ok > mx ? ok : mx;
            }
            lds.sort.key[i] = small_sort_key(reg[k], i);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t a1 = __shfl_xor(mn, o, 64), b1 = __shfl_xor(mx, o, 64);
        mn = a1 < mn ? a1 : mn;
        mx = b1 > mx ? b1 : mx;
    }
    if (lane == 0) {
        if (mn != ~0ULL) atomicMin(&s_mn, (unsigned long long)mn);
        if (mx != 0) atomicMax(&s_mx, (unsigned long long)mx);
    }
    const bool any_over = __syncthreads_or(over);                     // (B)
    if (t == 0) {
        ctl->min_now_key = s_mn;
        ctl->max_now_key = s_mx;
        ctl->span_overflow = any_over ? 1u : 0u;
    }

    // ---- 2. stable partition by region: rank, records to the scratch, runs, touched list
    RecC* recs = (RecC*)a.ra.rec;
#pragma unroll
    for (uint32_t k = 0; k < kSmallPer; ++k) {
        const uint32_t i = small_index(t, k);
        if (i < n) {
            pos[k] = small_rank(lds.sort.key, n, i);
            lds.sort.reg[pos[k]] = reg[k];
            recs[pos[k]] = rec[k];
        }
    }
    __syncthreads();                                                  // (C)
    bool head[kSmallPer];
    uint32_t hrank[kSmallPer], hreg[kSmallPer];
#pragma unroll
    for (uint32_t k = 0; k < kSmallPer; ++k) {
        const uint32_t p = small_index(t, k);             // a sorted position now
        head[k] = small_head(lds.sort.reg, n, p);
        hreg[k] = p < n ? lds.sort.reg[p] : 0u;
        const uint64_t m = __ballot(head[k]);
        hrank[k] = popc_below(m);
        if (lane == 0) lds.sort.wcnt[small_head_wave(p)] = (uint32_t)__popcll(m);
        if (head[k]) a.rstart[hreg[k]] = p;
        if (small_tail(lds.sort.reg, n, p)) a.rend[hreg[k]] = p + 1;
    }
    __syncthreads();                                                  // (D)
#pragma unroll
    for (uint32_t k = 0; k < kSmallPer; ++k) {
        const uint32_t p = small_index(t, k);
        if (head[k]) a.order[small_head_base(lds.sort.wcnt, p) + hrank[k]] = hreg[k];
    }
    if (t == 0) {
        uint32_t tot = 0;
        for (uint32_t w = 0; w < kSmallHeadWaves; ++w) tot += lds.sort.wcnt[w];
        a.order[a.ra.n_regions] = tot;
        s_tot = tot;
    }
    __syncthreads();                                                  // (E)

    // ---- 3. the touched regions over the waves, each decided by the region code
    const uint32_t tot = s_tot;
    for (uint32_t g = small_wave_first(wid); g < tot; g += small_wave_step()) {
        region_body_t<CodecC, uint32_t, true>(a.ra, g, lds.tab[wid]);
        wave_fence();
    }
    __syncthreads();                                                  // (F)

    // ---- 4. the control block, as the pipeline's kernels and k_stats_reduce leave it
    if (t == 0) {
        BatchCtl c;
        c.base_ms = base;
        c.min_now_key = s_mn;
        c.max_now_key = s_mx;
        c.span_overflow = any_over ? 1u : 0u;
        c.n_esc = ld_agent(&ctl->n_esc);
        c.allowed = ld_agent(stats + kStAllowed);
        c.distinct = ld_agent(stats + kStDistinct);
        c.invalid = ld_agent(stats + kStInvalid);
        c.cap_err = ld_agent(stats + kStCapErr);
        c.regions = ld_agent(stats + kStRegions);
        c.cache_hits = ld_agent(stats + kStCacheHits);
        for (int k = 0; k < 4; ++k) c.grow[k] = ld_agent(&ctl->grow[k]);
        c.table_bytes = ld_agent(stats + kStTableBytes);
        c.n_normal = n;
        c.n_hot = 0;
        c.internal_err = ld_agent(&ctl->internal_err);
        c.n_walk = 0;
        *ctl = c;
        *a.ctl_out = c;
    }

    // ---- 5. results back at their arrival indices
    const uint32_t* res = (const uint32_t*)a.ra.res;
#pragma unroll
    for (uint32_t k = 0; k < kSmallPer; ++k) {
        const uint32_t i = small_index(t, k);
        if (i < n) {
            const uint32_t j = pos[k], v = res[j];
            const bool esc = (uint64_t)v == kResEscape;
            a.allowed[i] = esc ? (uint8_t)0 : (uint8_t)(v & 1u);
            a.remaining[i] = esc ? a.ra.ext[j] : (int64_t)(v >> 1) - kResBias;
            if (a.tokens_out) a.tokens_out[i] = a.ra.tok[j];
        }
    }
}

hipError_t launch_small_batch(const SmallArgs& a, hipStream_t s) {
    if (a.n == 0 || a.n > kSmallMax) return hipErrorInvalidValue;
    if (a.ra.cache) hipLaunchKernelGGL(k_small_batch<true>, dim3(1), dim3(kSmallThreads), 0, s, a);
    else hipLaunchKernelGGL(k_small_batch<false>, dim3(1), dim3(kSmallThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace rl
