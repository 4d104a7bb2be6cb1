// rl_state.hip — state export, import (and rl_put_keys), table growth and the TTL sweep. What a
// slot holds, which of its buckets are live and how a region is rebuilt: rl_table.hpp.
#include "rl_table.hpp"

#pragma clang fp contract(off)

namespace rl {

// Export: one thread per slot of one limiter's table; every bucket live at `now` becomes one
// Redis-layout entry (SW: "rl:<key>:<W>" counters, deadline last INCR + w; TB: "tb:<key>",
// deadline last_refill + 2w), compacted through one counter. The host sorts the entries.
__global__ __launch_bounds__(256) void k_export(const Slot* __restrict__ tab, uint64_t n_slots,
                                                DevLimiter L, uint16_t lim, int64_t now,
                                                StateRec* __restrict__ out, uint32_t cap,
                                                uint32_t* count) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    const Slot v = tab[i];
    const LiveBuckets lb = live_buckets(L, v, now);
    if (lb.n == 0) return;
    const uint32_t k = atomicAdd(count, lb.n);
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) {               // (the older SW bucket first)
        if (j >= lb.n || k + j >= cap) continue;
        StateRec e{};
        e.key_hash = unmix64(v.tag); e.limiter = lim;
        e.expire_at_ms = lb.deadline[j];
        e.kind = L.algo == kAlgoTB ? 1 : 0;
        if (e.kind) { e.tokens = __longlong_as_double((long long)v.a); e.last_refill_ms = lb.start[j]; }
        else { e.window_start_ms = lb.start[j]; e.count = lb.count[j]; }
        out[k + j] = e;
    }
}

// Import: one wave per region that receives entries. The region's present slots are
// staged and rebuilt, then its keys are applied in order: replace the slot holding the
// key's tag, else claim the first free slot of the key's probe sequence (stage_put,
// rl_table.hpp). rl_put_keys runs the same kernel with the images' local-cache words (a.xw);
// the state import writes 0.
__global__ __launch_bounds__(64) void k_import(ImportArgs a) {
    __shared__ RegionStage S;
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    if (g >= a.n_groups) return;
    Slot* tab = (Slot*)(uintptr_t)a.region_addr[g];
    const int algo = a.group_algo[g];
    uint64_t* xt = (uint64_t*)(uintptr_t)a.xregion_addr[g];
    stage_clear(S, lane);
    stage_region(tab, xt, lane,
                 [&](const Slot& v, uint64_t x) { return slot_holds_state(algo, v, x); },
                 [&](const Slot&) -> RegionStage& { return S; });
    for (uint32_t j = a.group_off[g]; j < a.group_off[g + 1]; ++j) {
        const Slot im = a.img[j];
        const uint64_t x = a.xw ? a.xw[j] : 0;        // (rl_put_keys carries the cache word)
        if (!stage_put(S, im, x, lane) && lane == 0) atomicAdd(a.fail, 1u);
    }
    write_region(S, tab, xt, lane);
}

// Table growth (rl_grow_limiter): old region r of a limiter with 2^(k_new-1) regions splits
// into new regions 2r and 2r+1 by the next tag bit (region_local with one more bit); every
// slot holding state keeps its words and is re-inserted from its home in its new region.
// One wave per old region; each new region is written whole (free slots as zeros).
__global__ __launch_bounds__(64) void k_grow(const Slot* __restrict__ old_tab, const uint64_t* old_x,
                                             Slot* __restrict__ new_tab, uint64_t* new_x,
                                             uint64_t n_old, int shard_bits, int k_new, int algo) {
    __shared__ RegionStage S[2];
    constexpr uint32_t NS = kRegionSlots;
    const uint32_t lane = threadIdx.x;
    const uint64_t r = blockIdx.x;
    if (r >= n_old) return;
    stage_clear(S[0], lane); stage_clear(S[1], lane);
    stage_region(old_tab + r * NS, old_x ? old_x + r * NS : nullptr, lane,
                 [&](const Slot& v, uint64_t x) { return slot_holds_state(algo, v, x); },
                 [&](const Slot& v) -> RegionStage& { return S[region_local(v.tag, shard_bits, k_new) & 1u]; });
    write_region(S[0], new_tab + (2 * r) * NS, new_x ? new_x + (2 * r) * NS : nullptr, lane);
    write_region(S[1], new_tab + (2 * r + 1) * NS, new_x ? new_x + (2 * r + 1) * NS : nullptr, lane);
}

// TTL sweep: one wave per region; every used slot none of whose buckets is live at `now`
// (slot_live, the criterion a batch's region load applies) is dropped and the region is
// rebuilt (no tombstone survives a sweep). One counter atomic per wave.
__global__ __launch_bounds__(64) void k_sweep(uint64_t n_regions, DevLimiter L, int64_t now,
                                              uint32_t* count) {
    __shared__ RegionStage S;
    const uint32_t lane = threadIdx.x;
    const uint64_t r = blockIdx.x;
    if (r >= n_regions) return;
    const TableRegion R = table_region_at(L, r * kRegionSlots);
    stage_clear(S, lane);
    uint32_t dead = stage_region(R.tab, R.xtab, lane,
                                 [&](const Slot& v, uint64_t x) { return slot_live(L, v, now, x); },
                                 [&](const Slot&) -> RegionStage& { return S; });
    write_region(S, R.tab, R.xtab, lane);
    for (int o = 32; o > 0; o >>= 1) dead += __shfl_xor(dead, o, 64);
    if (lane == 0 && dead) atomicAdd(count, dead);
}

hipError_t launch_export(const Slot* table, uint64_t n_slots, const DevLimiter& L, uint16_t lim,
                         int64_t now_ms, StateRec* out, uint32_t cap, uint32_t* count,
                         hipStream_t s) {
    const uint64_t blocks = (n_slots + 255) / 256;
    hipLaunchKernelGGL(k_export, dim3((uint32_t)blocks), dim3(256), 0, s, table, n_slots, L, lim,
                       now_ms, out, cap, count);
    return hipGetLastError();
}

hipError_t launch_import(const ImportArgs& a, hipStream_t s) {
    if (a.n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(k_import, dim3(a.n_groups), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_grow(const Slot* old_tab, const uint64_t* old_x, Slot* new_tab, uint64_t* new_x,
                       uint64_t n_old_regions, int shard_bits, int k_new, int algo, hipStream_t s) {
    if (n_old_regions == 0) return hipSuccess;
    hipLaunchKernelGGL(k_grow, dim3((uint32_t)n_old_regions), dim3(64), 0, s, old_tab, old_x, new_tab,
                       new_x, n_old_regions, shard_bits, k_new, algo);
    return hipGetLastError();
}

hipError_t launch_sweep(const DevLimiter& L, uint64_t n_slots, int64_t now_ms, uint32_t* count,
                        hipStream_t s) {
    const uint64_t regions = n_slots / kRegionSlots;
    if (regions == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sweep, dim3((uint32_t)regions), dim3(64), 0, s, regions, L, now_ms, count);
    return hipGetLastError();
}

}  // namespace rl
