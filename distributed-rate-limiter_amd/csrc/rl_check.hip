// rl_check.hip — the read-only check of a table's slot invariants (rl_check_limiter(_device),
// rl_check_table_device, rl_check_images(_device); include/rl_engine.h). The rules are in
// rl_check.hpp; DESIGN.md §4 "Checking a table" states them and this pass' cost.
//
// k_check_regions: one wave per region, the waves of a persistent grid striding over the region
// range. Lane l reads slots j * 64 + l, j = 0..3, each as two 16-B loads plus its cache word
// (quad_load). Four ballots of slot_free build the region's 256-bit free map, which every lane
// then holds whole; a slot's reachability is mask arithmetic on it (check_unreachable: no loop
// over the chain). Duplicates: the wave stages the region's 256 tags and last-write times in LDS
// once (4 KB per wave) and every lane compares its four tags with the tag of every used slot of a
// lower index, read as a broadcast (at most 255 LDS reads and 1020 compares per lane and region,
// whatever the table holds); only a matching tag reads the other copy's time.
// Every class' slots are a ballot per row, so the counts are wave-uniform popcounts, kept by the
// lane whose index is the class id; a wave adds its sums at the end of its loop with one atomic
// per non-zero counter, and the first positions with one atomicMin per class that occurred, so
// the report does not depend on the launch geometry.
// Nothing read from the table is used as an address: a tag only feeds comparisons and slot
// indices are masked with & 255, so garbage input cannot make the pass read outside
// [tab, tab + n_regions * 256) and the cache words beside it.
//
// k_check_images: one lane per image (three 16-B loads), the value classes with the image's
// limiter's constants, accumulated the same way; first[] holds image indices.
#include "rl_check.hpp"
#include "rl_table.hpp"

#pragma clang fp contract(off)

namespace rl {

static_assert(kCheckRegionSlots == kRegionSlots && kCheckDeadMark == kDeadMark &&
              kCheckAlgoSW == kAlgoSW && kCheckAlgoTB == kAlgoTB, "rl_check.hpp restates rl_device.hpp");
static_assert(kCrWords == 7 + 2 * kCheckClasses && kCrViolations == 7, "rl_check_report layout");

namespace {

constexpr int kCheckThreads = 256;                // four regions per workgroup at a time
constexpr int kCheckWaves = kCheckThreads / 64;
constexpr uint32_t kCheckPerCu = 8;               // workgroups per CU of the persistent grid
constexpr uint32_t kRows = kRegionSlots / 64;

// A wave's sums over its loop: lane i < kCrViolations keeps scalar counter i, lane c keeps
// class c's count and first position (both arrays have kCheckClasses <= 64 entries).
struct CheckAcc {
    uint64_t scalar = 0, viol = 0, first = kCheckNone;
};

__device__ inline void acc_scalar(CheckAcc& A, uint32_t lane, uint32_t word, uint64_t n) {
    if (lane == word) A.scalar += n;
}
// the slots of class `cls` among one row of 64 positions starting at `pos0`
__device__ inline void acc_class(CheckAcc& A, uint32_t lane, uint32_t cls, uint64_t ballot, uint64_t pos0) {
    if (ballot == 0) return;                       // (wave-uniform)
    if (lane == cls) {
        A.viol += (uint64_t)__builtin_popcountll(ballot);
        const uint64_t p = pos0 + (uint64_t)__builtin_ctzll(ballot);
        if (p < A.first) A.first = p;
    }
}
__device__ inline void acc_flush(const CheckAcc& A, uint32_t lane, unsigned long long* out) {
    if (lane < kCrViolations && A.scalar) atomicAdd(out + lane, (unsigned long long)A.scalar);
    if (lane < kCheckClasses && A.viol) {
        atomicAdd(out + kCrViolations + lane, (unsigned long long)A.viol);
        atomicMin(out + kCrFirst + lane, (unsigned long long)A.first);
    }
}

__global__ __launch_bounds__(kCheckThreads) void k_check_regions(CheckArgs a) {
    __shared__ uint64_t s_tag[kCheckWaves][kRegionSlots];
    __shared__ int64_t s_lw[kCheckWaves][kRegionSlots];       // last write; kNoWrite: no bucket state
    constexpr int64_t kNoWrite = INT64_MIN;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const CheckLimiter CL{a.algo, a.window_ms, a.ttl_ms};
    CheckAcc A;
    const uint64_t stride = (uint64_t)gridDim.x * kCheckWaves;
    // (wave-uniform trip count: the ballots below need every lane)
    for (uint64_t i = (uint64_t)blockIdx.x * kCheckWaves + wid; i < a.m; i += stride) {
        const uint64_t r = a.region_begin + i;     // < 2^region_bits (the launcher clipped the range)
        const TableRegion R{as_global((Slot*)a.tab + r * kRegionSlots),
                            a.xtab ? as_global((uint64_t*)a.xtab + r * kRegionSlots) : nullptr};
        QuadSlot s[kRows];
#pragma unroll
        for (uint32_t j = 0; j < kRows; ++j) s[j] = quad_load(R, j * 64 + lane);
        CheckFreeMap F;
        bool used[kRows];
        int64_t lw[kRows];
        uint64_t n_used = 0, n_state = 0, n_cache = 0;
#pragma unroll
        for (uint32_t j = 0; j < kRows; ++j) {
            used[j] = check_used(s[j].lo.x, s[j].lo.y, s[j].hi.x, s[j].hi.y, s[j].x);
            const uint64_t um = __ballot(used[j]);
            F.w[j] = ~um;
            n_used += (uint64_t)__builtin_popcountll(um);
            n_state += (uint64_t)__builtin_popcountll(
                __ballot(used[j] && check_holds_state(a.algo, s[j].hi.x, s[j].hi.y, s[j].x)));
            n_cache += (uint64_t)__builtin_popcountll(__ballot(s[j].x != 0));
            if (!check_last_write(CL, s[j].lo.y, s[j].hi.x, s[j].hi.y, &lw[j])) lw[j] = kNoWrite;
            s_tag[wid][j * 64 + lane] = s[j].lo.x;
            s_lw[wid][j * 64 + lane] = lw[j];
        }
        wave_fence();
        // duplicates: my tags against the tag of every used slot of a lower index
        bool dup[kRows] = {false, false, false, false};
#pragma unroll
        for (uint32_t jt = 0; jt < kRows; ++jt) {
            for (uint64_t um = ~F.w[jt]; um; um &= um - 1) {       // (wave-uniform) the used slots
                const uint32_t t = jt * 64 + (uint32_t)__builtin_ctzll(um);
                const uint64_t tt = s_tag[wid][t];                 // broadcast read
#pragma unroll
                for (uint32_t j = jt; j < kRows; ++j) {
                    if (s[j].lo.x == tt && t < j * 64 + lane && lw[j] != kNoWrite) {   // (rare)
                        const int64_t other = s_lw[wid][t];
                        dup[j] |= other != kNoWrite && check_copies_conflict(lw[j], other, CL.ttl_ms);
                    }
                }
            }
        }
        wave_fence();                                              // the next region overwrites the stage
        uint64_t n_bad = 0;
#pragma unroll
        for (uint32_t j = 0; j < kRows; ++j) {
            const uint32_t slot = (j * 64 + lane) & (kRegionSlots - 1);
            uint32_t m = 0;
            if (used[j]) {
                m = check_slot_values(CL, s[j].lo.x, s[j].lo.y, s[j].hi.x, s[j].hi.y, s[j].x);
                if (check_region_of(s[j].lo.x, a.shard_bits, a.region_bits) != (uint32_t)r) m |= 1u << kCkWrongRegion;
                if (check_unreachable(F, s[j].lo.x, slot)) m |= 1u << kCkUnreachable;
                if (dup[j]) m |= 1u << kCkDuplicate;
            }
            const uint64_t bad = __ballot(m != 0);
            if (bad == 0) continue;                                // (wave-uniform) the healthy case
            n_bad += (uint64_t)__builtin_popcountll(bad);
            const uint64_t pos0 = check_pos(r, j * 64);
#pragma unroll
            for (uint32_t c = 0; c <= kCkTbFlags; ++c) acc_class(A, lane, c, __ballot((m >> c) & 1u), pos0);
        }
        acc_scalar(A, lane, kCrUsed, n_used);
        acc_scalar(A, lane, kCrState, n_state);
        acc_scalar(A, lane, kCrTomb, n_used - n_state);
        acc_scalar(A, lane, kCrCache, n_cache);
        acc_scalar(A, lane, kCrBad, n_bad);
    }
    acc_flush(A, lane, a.out);
}

__global__ __launch_bounds__(kCheckThreads) void k_check_images(CheckImgArgs a) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    RL_GLOBAL const u64x2_t* in = (RL_GLOBAL const u64x2_t*)as_global(a.in);
    CheckAcc A;
    const uint64_t stride = (uint64_t)gridDim.x * kCheckThreads;
    for (uint64_t base = (uint64_t)blockIdx.x * kCheckThreads + wid * 64; base < a.n; base += stride) {
        const uint64_t i = base + lane;
        uint32_t m = 0;
        bool used = false, state = false, cache = false;
        if (i < a.n) {
            const u64x2_t w0 = in[3 * i], w1 = in[3 * i + 1], w2 = in[3 * i + 2];
            const uint64_t tag = mix64(w0.x);
            const uint32_t lim = (uint32_t)(w2.y & 0xFFFFu);
            used = check_used(tag, w0.y, w1.x, w1.y, w2.x);
            cache = w2.x != 0;
            if ((w2.y >> 16) != 0) m |= 1u << kCkImageReserved;
            if (lim >= a.n_lim) {
                m |= 1u << kCkImageLimiter;
            } else {
                const CheckLimiter CL{a.lims[lim].algo, a.lims[lim].window_ms, a.lims[lim].ttl_ms};
                state = used && check_holds_state(CL.algo, w1.x, w1.y, w2.x);
                if (used) m |= check_slot_values(CL, tag, w0.y, w1.x, w1.y, w2.x) & ~(1u << kCkDeadMark);
            }
        }
        const uint64_t um = __ballot(used), sm = __ballot(state);
        acc_scalar(A, lane, kCrUsed, (uint64_t)__builtin_popcountll(um));
        acc_scalar(A, lane, kCrState, (uint64_t)__builtin_popcountll(sm));
        acc_scalar(A, lane, kCrTomb, (uint64_t)__builtin_popcountll(um & ~sm));
        acc_scalar(A, lane, kCrCache, (uint64_t)__builtin_popcountll(__ballot(cache)));
        const uint64_t bad = __ballot(m != 0);
        if (bad == 0) continue;                                    // (wave-uniform)
        acc_scalar(A, lane, kCrBad, (uint64_t)__builtin_popcountll(bad));
#pragma unroll
        for (uint32_t c = kCkSwStart; c <= kCkImageReserved; ++c)
            acc_class(A, lane, c, __ballot((m >> c) & 1u), a.index_base + base);
    }
    acc_flush(A, lane, a.out);
}

// regions / slots as given, every counter 0, every first position "none"
__global__ void k_check_init(unsigned long long* out, unsigned long long regions, unsigned long long slots) {
    const uint32_t i = threadIdx.x;
    if (i >= kCrWords) return;
    out[i] = i == kCrRegions ? regions : i == kCrSlots ? slots : i >= kCrFirst ? kCheckNone : 0ULL;
}

}  // namespace

hipError_t launch_check_init(unsigned long long* out, uint64_t regions, uint64_t slots, hipStream_t s) {
    hipLaunchKernelGGL(k_check_init, dim3(1), dim3(64), 0, s, out, (unsigned long long)regions,
                       (unsigned long long)slots);
    return hipGetLastError();
}

hipError_t launch_check_regions(const CheckArgs& a, hipStream_t s) {
    if (a.m == 0) return hipSuccess;
    const uint64_t blocks = (a.m + kCheckWaves - 1) / kCheckWaves;
    const uint32_t grid = persistent_grid((uint32_t)std::min<uint64_t>(blocks, 1u << 30), kCheckPerCu);
    hipLaunchKernelGGL(k_check_regions, dim3(grid), dim3(kCheckThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_check_images(const CheckImgArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint64_t blocks = (a.n + kCheckThreads - 1) / kCheckThreads;
    const uint32_t grid = persistent_grid((uint32_t)std::min<uint64_t>(blocks, 1u << 30), kCheckPerCu);
    hipLaunchKernelGGL(k_check_images, dim3(grid), dim3(kCheckThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace rl
