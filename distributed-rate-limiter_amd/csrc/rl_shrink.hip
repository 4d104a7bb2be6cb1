// rl_shrink.hip — table shrink (rl_shrink_plan / rl_shrink_limiter, include/rl_engine.h): the
// inverse of k_grow (rl_state.hip). The rules (how many halvings, how many passes):
// rl_shrink.hpp; how a region is staged and written back: rl_table.hpp.
//
//   k_shrink_count   one wave per region, as k_sweep: the region's slots live at `now`
//                    (slot_live, the sweep's keep rule) and its used slots, one word each per
//                    region. No atomic.
//   k_shrink_totals  level 0 of the reduction: the largest per-region live count and the two
//                    totals, one workgroup partial each, then three atomics per workgroup.
//   k_shrink_fold    one further level: out[r] = in[2r] + in[2r+1] (regions 2r and 2r+1 are
//                    region r of the table with one region bit less) and the level's maximum.
//                    At most kShrinkLevels - 1 launches over n/2, n/4, ... words: tiny beside
//                    the count's pass over the table.
//   k_shrink_merge   one wave per DESTINATION region r': the kept slots of the source regions
//                    r' << s ... (r' << s) + 2^s - 1 (s <= 3: at most 64 KB per wave) go into one
//                    LDS stage, each from its home, and the region is written whole (free slots
//                    as zeros, cache words to the cache table). The plan has proved that the
//                    kept slots of one destination region number at most kShrinkFillMax; the
//                    insert is bounded all the same (stage_insert_bounded: one turn of the
//                    region) and a slot that finds no place is counted in *fail, on which the
//                    host discards the new table.
// Every loop here runs over an index range fixed at launch; none waits on table contents.
#include "rl_shrink.hpp"
#include "rl_table.hpp"

#pragma clang fp contract(off)

namespace rl {

static_assert(kShrinkRegionSlots == (uint32_t)kRegionSlots, "slots per region");
static_assert(kShrinkMinRegionBits == (uint32_t)kBinShift, "a limiter keeps one bin of regions");
static_assert(sizeof(ShrinkCtl::fullest) / sizeof(uint32_t) == kShrinkLevels, "fullest[]");

namespace {

constexpr int kFoldThreads = 256;
constexpr uint32_t kFoldBlocksMax = 1024;          // (bounds the atomics per level)

__device__ inline uint32_t wave_sum32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline uint32_t wave_max32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(64) void k_shrink_count(uint64_t n_regions, DevLimiter L, int64_t now,
                                                     uint32_t* __restrict__ kept,
                                                     uint32_t* __restrict__ used) {
    constexpr uint32_t NS = kRegionSlots;
    const uint32_t lane = threadIdx.x;
    const uint64_t r = blockIdx.x;
    if (r >= n_regions) return;
    const TableRegion R = table_region_at(L, r * NS);
    uint32_t k = 0, u = 0;
#pragma unroll
    for (uint32_t i = 0; i < NS / 64; ++i) {
        const Slot v = R.tab[lane + 64 * i];
        const uint64_t x = R.xtab ? R.xtab[lane + 64 * i] : 0;
        const bool in_use = !slot_free(v, x);
        u += in_use ? 1u : 0u;
        k += (in_use && slot_live(L, v, now, x)) ? 1u : 0u;
    }
    k = wave_sum32(k);
    u = wave_sum32(u);
    if (lane == 0) { kept[r] = k; used[r] = u; }
}

__global__ __launch_bounds__(kFoldThreads) void k_shrink_totals(const uint32_t* __restrict__ kept,
                                                                const uint32_t* __restrict__ used,
                                                                uint64_t n, ShrinkCtl* ctl) {
    __shared__ uint32_t s_max[kFoldThreads / 64];
    __shared__ unsigned long long s_kept[kFoldThreads / 64], s_used[kFoldThreads / 64];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t m = 0, k = 0, u = 0;                  // (one lane's share of <= 2^32 slots fits)
    for (uint64_t r = (uint64_t)blockIdx.x * kFoldThreads + threadIdx.x; r < n;
         r += (uint64_t)gridDim.x * kFoldThreads) {
        const uint32_t c = kept[r];
        m = c > m ? c : m;
        k += c;
        u += used[r];
    }
    m = wave_max32(m);
    unsigned long long k64 = k, u64 = u;           // (the totals may reach 2^24 regions x 256)
    for (int o = 32; o > 0; o >>= 1) {
        k64 += (unsigned long long)shfl64((int64_t)k64, (int)(lane ^ (uint32_t)o));
        u64 += (unsigned long long)shfl64((int64_t)u64, (int)(lane ^ (uint32_t)o));
    }
    if (lane == 0) { s_max[wid] = m; s_kept[wid] = k64; s_used[wid] = u64; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kFoldThreads / 64; ++w) {
            m = s_max[w] > m ? s_max[w] : m;
            k64 += s_kept[w];
            u64 += s_used[w];
        }
        if (m) atomicMax(&ctl->fullest[0], m);
        if (k64) atomicAdd(&ctl->kept, k64);
        if (u64) atomicAdd(&ctl->used, u64);
    }
}

__global__ __launch_bounds__(kFoldThreads) void k_shrink_fold(const uint32_t* __restrict__ in,
                                                              uint32_t* __restrict__ out,
                                                              uint64_t n_out, uint32_t* fullest) {
    __shared__ uint32_t s_max[kFoldThreads / 64];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t m = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * kFoldThreads + threadIdx.x; r < n_out;
         r += (uint64_t)gridDim.x * kFoldThreads) {
        const uint32_t c = in[2 * r] + in[2 * r + 1];
        out[r] = c;
        m = c > m ? c : m;
    }
    m = wave_max32(m);
    if (lane == 0) s_max[wid] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kFoldThreads / 64; ++w) m = s_max[w] > m ? s_max[w] : m;
        if (m) atomicMax(fullest, m);
    }
}

template <bool LIVE>
__global__ __launch_bounds__(64) void k_shrink_merge(const Slot* __restrict__ src_tab,
                                                     const uint64_t* __restrict__ src_x,
                                                     Slot* __restrict__ dst_tab, uint64_t* dst_x,
                                                     uint64_t n_dst, uint32_t s, DevLimiter L,
                                                     int64_t now, uint32_t* fail) {
    __shared__ RegionStage S;
    constexpr uint32_t NS = kRegionSlots;
    const uint32_t lane = threadIdx.x;
    const uint64_t rd = blockIdx.x;
    if (rd >= n_dst) return;
    stage_clear(S, lane);
    wave_fence();
    uint32_t lost = 0;
    const uint32_t n_src = 1u << s;                                  // <= 8 (launch_shrink_merge)
    for (uint32_t q = 0; q < n_src; ++q) {
        const uint64_t slot0 = ((rd << s) + q) * NS;                 // < (n_dst << s) * NS: inside src
        const Slot* tab = src_tab + slot0;
        const uint64_t* xt = src_x ? src_x + slot0 : nullptr;
        Slot img[NS / 64];
        uint64_t xim[NS / 64];
#pragma unroll
        for (uint32_t i = 0; i < NS / 64; ++i) {
            img[i] = tab[lane + 64 * i];
            xim[i] = xt ? xt[lane + 64 * i] : 0;
        }
#pragma unroll
        for (uint32_t i = 0; i < NS / 64; ++i) {
            bool keep = !slot_free(img[i], xim[i]);
            if (keep) keep = LIVE ? slot_live(L, img[i], now, xim[i]) : slot_holds_state(L.algo, img[i], xim[i]);
            if (keep && !stage_insert_bounded(S, img[i], xim[i])) ++lost;
        }
    }
    wave_fence();
    write_region(S, dst_tab + rd * NS, dst_x ? dst_x + rd * NS : nullptr, lane);
    lost = wave_sum32(lost);
    if (lane == 0 && lost) atomicAdd(fail, lost);
}

inline uint32_t fold_blocks(uint64_t n) {
    const uint64_t b = (n + kFoldThreads - 1) / kFoldThreads;
    return (uint32_t)(b < 1 ? 1 : b > kFoldBlocksMax ? kFoldBlocksMax : b);
}

}  // namespace

size_t shrink_scratch_bytes(uint64_t n_regions) {
    return sizeof(ShrinkCtl) + (size_t)n_regions * 3 * sizeof(uint32_t);
}
ShrinkScratch shrink_scratch_at(void* base, uint64_t n_regions) {
    ShrinkScratch sc;
    sc.ctl = (ShrinkCtl*)base;
    sc.kept = (uint32_t*)(sc.ctl + 1);
    sc.used = sc.kept + n_regions;
    sc.sums = sc.used + n_regions;                 // n/2 + n/4 + ... < n words
    return sc;
}

hipError_t launch_shrink_plan(const ShrinkScratch& sc, const DevLimiter& L, uint64_t n_regions,
                              uint32_t levels, int64_t now_ms, hipStream_t s) {
    if (n_regions == 0 || levels == 0 || levels > kShrinkLevels || (n_regions >> (levels - 1)) == 0)
        return hipErrorInvalidValue;
    hipError_t he = hipMemsetAsync(sc.ctl, 0, sizeof(ShrinkCtl), s);
    if (he != hipSuccess) return he;
    hipLaunchKernelGGL(k_shrink_count, dim3((uint32_t)n_regions), dim3(64), 0, s, n_regions, L, now_ms,
                       sc.kept, sc.used);
    hipLaunchKernelGGL(k_shrink_totals, dim3(fold_blocks(n_regions)), dim3(kFoldThreads), 0, s,
                       (const uint32_t*)sc.kept, (const uint32_t*)sc.used, n_regions, sc.ctl);
    const uint32_t* in = sc.kept;
    uint32_t* out = sc.sums;
    uint64_t n = n_regions;
    for (uint32_t i = 1; i < levels; ++i) {
        n >>= 1;                                   // >= 1 (checked above)
        hipLaunchKernelGGL(k_shrink_fold, dim3(fold_blocks(n)), dim3(kFoldThreads), 0, s, in, out, n,
                           &sc.ctl->fullest[i]);
        in = out;
        out += n;
    }
    return hipGetLastError();
}

hipError_t launch_shrink_merge(const Slot* src_tab, const uint64_t* src_x, Slot* dst_tab,
                               uint64_t* dst_x, uint64_t n_dst, uint32_t s, const DevLimiter& L,
                               int64_t now_ms, bool live_only, uint32_t* fail, hipStream_t st) {
    if (n_dst == 0 || s == 0 || s > kShrinkPassBits || n_dst > (1ull << 24) || (src_x == nullptr) != (dst_x == nullptr))
        return hipErrorInvalidValue;
    if (live_only)
        hipLaunchKernelGGL(k_shrink_merge<true>, dim3((uint32_t)n_dst), dim3(64), 0, st, src_tab, src_x,
                           dst_tab, dst_x, n_dst, s, L, now_ms, fail);
    else
        hipLaunchKernelGGL(k_shrink_merge<false>, dim3((uint32_t)n_dst), dim3(64), 0, st, src_tab, src_x,
                           dst_tab, dst_x, n_dst, s, L, now_ms, fail);
    return hipGetLastError();
}

}  // namespace rl
