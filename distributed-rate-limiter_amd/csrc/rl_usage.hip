// rl_usage.hip — census of one limiter's state table (rl_limiter_usage, rl_top_consumers,
// include/rl_engine.h): how full it is, how many keys are live / throttled at `now`, and the
// keys that have used most of their limit.
//
// Every kernel here is one read-only pass over the limiter's slots (grid-stride, a wave takes
// 64 consecutive slots = 2 KB at a time) that evaluates each slot with the engine's own peek
// code (tb_step / sw_step with kOpPeek, rl_device.hpp): the numbers are what RL_OP_PEEK would
// return for every key at `now`, for the slots live_buckets (rl_table.hpp) finds alive. No table
// word, cache word or batch scratch is written.
//
//   k_usage_census   the ~22 counters of rl_usage. Lanes keep their own sums over the whole
//                    loop (histogram bin b lives in lane b: one ballot + popcount per bin and
//                    step, no atomic), a wave reduces them once at the end, the workgroup adds
//                    its waves' sums in LDS and issues one 64-bit global atomic per non-zero
//                    counter. (Per-slot atomics would serialise on exhausted_keys and hist[15]:
//                    every throttled key lands there.)
//   k_usage_digits   one pass of the MSD radix select of rl_top_consumers: the keys still in
//                    play (composite C = used << 64 | ~key_hash with C >> top == prefix) are
//                    counted by their next 12-bit digit. The histogram is private to the
//                    workgroup in LDS (16 KB) and flushed with one global atomic per non-empty
//                    digit; lanes of a wave with equal digits merge before the LDS atomic (up to
//                    four leaders a step — after the first pass every survivor may share the
//                    same `used` — the rest add singly).
//   k_usage_compact  appends {key_hash, used} of every key with C >> top >= prefix (the cut bin
//                    and the fewer than k keys above it) to the candidate store, one global
//                    atomic per wave and step.
// The host (rl_engine_query.cpp) drives the passes, reads the histogram between them and orders the
// candidates.
#include "rl_table.hpp"

#pragma clang fp contract(off)

namespace rl {

namespace {

constexpr int kUsageThreads = 256;
constexpr int kUsageWaves = kUsageThreads / 64;
constexpr uint32_t kUsagePerCu = 8;                // workgroups per CU of the persistent grids

typedef unsigned __int128 u128;

struct UsageEval {
    bool used_slot;          // not free (a live key or a tombstone)
    bool blocked;            // its cache word rejects at now
    uint32_t redis;          // Redis keys live at now (SW: 0..2 buckets, TB: 0..1 hash)
    int64_t used;            // live (redis != 0): max - clamp(available, 0, max)
};

// Liveness is live_buckets (rl_table.hpp); `available` is the peek of the shared step functions.
__device__ inline UsageEval usage_eval(const DevLimiter& L, const Slot& v, uint64_t x, int64_t now) {
    UsageEval u;
    u.used_slot = !slot_free(v, x);
    u.blocked = x != 0 && now < (int64_t)x;
    u.used = 0;
    int64_t avail = 0;
    if (L.algo == kAlgoTB) {       // (live_buckets inside the branch: it folds to this algorithm's rule)
        u.redis = live_buckets(L, v, now).n;
        if (u.redis) avail = tb_step(L, kOpPeek, 1, now, v.a, v.b, v.c).remaining;
    } else {
        u.redis = live_buckets(L, v, now).n;
        if (u.redis) avail = sw_step(L, kOpPeek, 1, now, v.a, v.b, v.c).remaining;
    }
    if (u.redis) {
        if (avail < 0) avail = 0;                  // TB after time regression
        if (avail > L.max_permits) avail = L.max_permits;
        u.used = L.max_permits - avail;
    }
    return u;
}

__device__ inline uint64_t wave_sum64(uint64_t v, uint32_t lane) {
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)shfl64((int64_t)v, (int)(lane ^ (uint32_t)o));
    return v;
}

__device__ inline RL_GLOBAL const uint64_t* cache_words(const DevLimiter& L) {
    return L.cache_table ? as_global((const uint64_t*)L.cache_table) : nullptr;
}

// ---------------------------------------------------------------- census
__global__ __launch_bounds__(kUsageThreads) void k_usage_census(UsageScratch sc,
                                                                const Slot* __restrict__ tab,
                                                                uint64_t n_slots, DevLimiter L,
                                                                int64_t now) {
    __shared__ unsigned long long s_part[kUsageWaves][kUcWords];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    RL_GLOBAL const uint64_t* xtab = cache_words(L);
    uint64_t c_used = 0, c_live = 0, c_redis = 0, c_exh = 0, c_blk = 0, c_perm = 0;
    uint64_t c_hist = 0;                           // lane b < kUsageBins: hist[b]
    const uint64_t stride = (uint64_t)gridDim.x * kUsageThreads;
    // (wave-uniform trip count: the ballots below need every lane)
    for (uint64_t base = (uint64_t)blockIdx.x * kUsageThreads + wid * 64; base < n_slots; base += stride) {
        const uint64_t i = base + lane;
        bool live = false;
        uint32_t bin = 0;
        if (i < n_slots) {
            const Slot v = tab[i];
            const uint64_t x = xtab ? xtab[i] : 0;
            const UsageEval u = usage_eval(L, v, x, now);
            c_used += u.used_slot ? 1u : 0u;
            c_blk += u.blocked ? 1u : 0u;
            c_redis += u.redis;
            if (u.redis) {
                live = true;
                c_live += 1;
                c_perm += (uint64_t)u.used;
                const bool full = u.used == L.max_permits;
                c_exh += full ? 1u : 0u;
                bin = full ? kUsageBins - 1 : (uint32_t)((u.used * (int64_t)kUsageBins) / L.max_permits);
            }
        }
#pragma unroll
        for (uint32_t b = 0; b < kUsageBins; ++b) {
            const uint32_t cnt = (uint32_t)__builtin_popcountll(__ballot(live && bin == b));
            if (lane == b) c_hist += cnt;
        }
    }
    c_used = wave_sum64(c_used, lane); c_live = wave_sum64(c_live, lane);
    c_redis = wave_sum64(c_redis, lane); c_exh = wave_sum64(c_exh, lane);
    c_blk = wave_sum64(c_blk, lane); c_perm = wave_sum64(c_perm, lane);
    if (lane == 0) {
        s_part[wid][kUcUsedSlots] = c_used; s_part[wid][kUcLive] = c_live;
        s_part[wid][kUcRedis] = c_redis; s_part[wid][kUcExhausted] = c_exh;
        s_part[wid][kUcCacheBlocked] = c_blk; s_part[wid][kUcUsedPermits] = c_perm;
    }
    if (lane < kUsageBins) s_part[wid][kUcHist + lane] = c_hist;
    __syncthreads();
    if (threadIdx.x < kUcWords) {
        unsigned long long t = 0;
        for (int w = 0; w < kUsageWaves; ++w) t += s_part[w][threadIdx.x];
        if (t) atomicAdd(sc.counters + threadIdx.x, t);
    }
}

// ---------------------------------------------------------------- top consumers
// The slot's composite sort key, if it takes part: live, used >= min_used, C >> top matching
// (EQ) or at least (!EQ) the prefix.
template <bool EQ>
__device__ inline bool usage_composite(const DevLimiter& L, const Slot& v, int64_t now,
                                       const UsageSel& sel, u128& C, int64_t& used) {
    const UsageEval u = usage_eval(L, v, 0, now);
    if (!u.redis || u.used < sel.min_used) return false;
    used = u.used;
    C = ((u128)(uint64_t)u.used << 64) | (u128)~unmix64(v.tag);
    const u128 prefix = ((u128)sel.prefix_hi << 64) | (u128)sel.prefix_lo;
    const u128 head = C >> sel.top;
    return EQ ? head == prefix : head >= prefix;
}

__global__ __launch_bounds__(kUsageThreads) void k_usage_digits(UsageScratch sc,
                                                                const Slot* __restrict__ tab,
                                                                uint64_t n_slots, DevLimiter L,
                                                                int64_t now, UsageSel sel) {
    __shared__ uint32_t s_hist[kUsageDigits];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (uint32_t b = threadIdx.x; b < kUsageDigits; b += kUsageThreads) s_hist[b] = 0;
    __syncthreads();
    const uint32_t dmask = (1u << (sel.top - sel.pos)) - 1;
    const uint64_t stride = (uint64_t)gridDim.x * kUsageThreads;
    for (uint64_t base = (uint64_t)blockIdx.x * kUsageThreads + wid * 64; base < n_slots; base += stride) {
        const uint64_t i = base + lane;
        bool m = false;
        uint32_t d = 0;
        if (i < n_slots) {
            u128 C;
            int64_t used;
            m = usage_composite<true>(L, tab[i], now, sel, C, used);
            if (m) d = (uint32_t)(C >> sel.pos) & dmask;
        }
        uint64_t todo = __ballot(m);
        for (int r = 0; r < 4 && todo; ++r) {      // (wave-uniform)
            const int leader = __builtin_ctzll(todo);
            const uint32_t dl = (uint32_t)__builtin_amdgcn_readlane((int)d, leader);
            const bool eq = m && d == dl;
            const uint64_t same = __ballot(eq);
            if ((int)lane == leader) atomicAdd(&s_hist[dl], (uint32_t)__builtin_popcountll(same));
            if (eq) m = false;
            todo &= ~same;
        }
        if (m) atomicAdd(&s_hist[d], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kUsageDigits; b += kUsageThreads) {
        const uint32_t c = s_hist[b];
        if (c) atomicAdd(sc.hist + b, (unsigned long long)c);
    }
}

__global__ __launch_bounds__(kUsageThreads) void k_usage_compact(UsageScratch sc,
                                                                 const Slot* __restrict__ tab,
                                                                 uint64_t n_slots, DevLimiter L,
                                                                 int64_t now, UsageSel sel) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t stride = (uint64_t)gridDim.x * kUsageThreads;
    for (uint64_t base = (uint64_t)blockIdx.x * kUsageThreads + wid * 64; base < n_slots; base += stride) {
        const uint64_t i = base + lane;
        bool m = false;
        UsageCand c{0, 0};
        if (i < n_slots) {
            u128 C;
            const Slot v = tab[i];
            m = usage_composite<false>(L, v, now, sel, C, c.used);
            c.key_hash = unmix64(v.tag);
        }
        const uint64_t mask = __ballot(m);
        if (mask == 0) continue;                   // (wave-uniform)
        const int leader = __builtin_ctzll(mask);
        uint64_t at = 0;
        if ((int)lane == leader)
            at = atomicAdd(sc.counters + kUsageCandCount, (unsigned long long)__builtin_popcountll(mask));
        at = readlane64(at, (uint32_t)leader) + popc_below(mask);
        // the host's cut keeps the store within bounds; a count beyond it reports RL_E_INTERNAL
        if (m && at < kUsageStore) sc.cand[at] = c;
    }
}

uint32_t usage_grid(uint64_t n_slots) {
    const uint64_t blocks = (n_slots + kUsageThreads - 1) / kUsageThreads;
    return persistent_grid((uint32_t)std::min<uint64_t>(blocks, 1u << 30), kUsagePerCu);
}

}  // namespace

size_t usage_scratch_bytes() {
    return 32 * sizeof(unsigned long long) + kUsageDigits * sizeof(unsigned long long) +
           (size_t)kUsageStore * sizeof(UsageCand);
}

UsageScratch usage_scratch_at(void* base) {
    UsageScratch sc;
    sc.counters = (unsigned long long*)base;
    sc.hist = sc.counters + 32;
    sc.cand = (UsageCand*)(sc.hist + kUsageDigits);
    return sc;
}

hipError_t launch_usage_census(const UsageScratch& sc, const Slot* table, uint64_t n_slots,
                               const DevLimiter& L, int64_t now_ms, hipStream_t s) {
    if (n_slots == 0) return hipSuccess;
    hipLaunchKernelGGL(k_usage_census, dim3(usage_grid(n_slots)), dim3(kUsageThreads), 0, s, sc, table,
                       n_slots, L, now_ms);
    return hipGetLastError();
}

hipError_t launch_usage_digits(const UsageScratch& sc, const Slot* table, uint64_t n_slots,
                               const DevLimiter& L, int64_t now_ms, const UsageSel& sel, hipStream_t s) {
    if (n_slots == 0) return hipSuccess;
    hipLaunchKernelGGL(k_usage_digits, dim3(usage_grid(n_slots)), dim3(kUsageThreads), 0, s, sc, table,
                       n_slots, L, now_ms, sel);
    return hipGetLastError();
}

hipError_t launch_usage_compact(const UsageScratch& sc, const Slot* table, uint64_t n_slots,
                                const DevLimiter& L, int64_t now_ms, const UsageSel& sel, hipStream_t s) {
    if (n_slots == 0) return hipSuccess;
    hipLaunchKernelGGL(k_usage_compact, dim3(usage_grid(n_slots)), dim3(kUsageThreads), 0, s, sc, table,
                       n_slots, L, now_ms, sel);
    return hipGetLastError();
}

}  // namespace rl
