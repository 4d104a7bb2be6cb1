// rl_report.hip — per-limiter counts of a finished batch (rl_tally_batch, include/rl_engine.h):
// for every request its row and class (rl_report.hpp) from the batch's own arrays, summed into
// out[256] rows of 10 counters. Read-only on the batch; nothing of the engine's is touched.
//
// One persistent grid-stride kernel. A workgroup of 256 threads takes tiles of 2048 requests and
// keeps all 256 x 10 counters in LDS (20 KB). A wave folds the 64 requests of one load round per
// DISTINCT ROW PRESENT: it takes the first remaining lane's row, ballots the lanes with that
// row, popcounts the class ballots, wave-reduces the two permit sums (in one 32-bit reduction
// when every permit count is small) and lets that one lane add the non-zero results to the
// row's LDS cells; then the same for the lanes that are left. Real
// traffic has 1-10 rows per wave; 64 distinct rows cost 64 rounds and are still exact. When the
// workgroup ends it adds its non-zero cells to `out` with 64-bit global atomics, so the global
// atomics number at most 2560 per workgroup whatever n is, never one per request or per wave
// (one contended word takes about 88 returning adds per microsecond).
#include "rl_kcommon.hpp"
#include "rl_report.hpp"

namespace rl {

namespace {

constexpr int kTallyThreads = 256;
constexpr int kTallyTile = 2048;                   // requests a workgroup takes at a time
constexpr int kTallyPerThread = kTallyTile / kTallyThreads;
constexpr uint32_t kTallyPerCu = 6;                // 20 KB of LDS each
constexpr uint32_t kTallyCells = kTallyRows * kTcCols;

constexpr uint32_t kSmallPermits = 1024;           // 64 x 1023 < 2^16

__device__ inline uint64_t wave_sum64(uint64_t v) {
    return wave_reduce_dpp(v, [](uint64_t x, uint64_t y) { return x + y; });
}
__device__ inline uint32_t wave_sum32(uint32_t v) {
    return wave_reduce_dpp(v, [](uint32_t x, uint32_t y) { return x + y; });
}

// The requests of one load round of a wave (a lane's is `active` or not) into the LDS cells.
// Every lane of the wave calls this together.
__device__ inline void wave_fold(unsigned long long* s_cell, uint32_t lane, bool active, uint32_t row,
                                 uint32_t cls, bool over_max, uint32_t permits) {
    uint64_t todo = __ballot(active);
    while (todo) {                                                   // wave-uniform
        const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
        const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)row, (int)lead);
        const bool mine = active && row == r;
        const uint64_t m = __ballot(mine);
        uint32_t c[kRcClasses];
#pragma unroll
        for (uint32_t k = 0; k < kRcClasses; ++k) c[k] = (uint32_t)__popcll(__ballot(mine && cls == k));
        const uint32_t n_over = (uint32_t)__popcll(__ballot(mine && over_max));
        uint64_t pa = 0, pd = 0;                                     // permits > 0 in both classes
        if (c[kRcAllowed] | c[kRcDenied]) {
            const bool pa_mine = mine && cls == kRcAllowed, pd_mine = mine && cls == kRcDenied;
            if (__ballot((pa_mine || pd_mine) && permits >= kSmallPermits) == 0) {
                // the usual case, every permit count small: 64 of them sum to less than 2^16, so
                // both sums share one 32-bit reduction (allowed low half, denied high half)
                const uint32_t both = wave_sum32(pa_mine ? permits : pd_mine ? permits << 16 : 0u);
                pa = both & 0xFFFFu;
                pd = both >> 16;
            } else {
                if (c[kRcAllowed]) pa = wave_sum64(pa_mine ? (uint64_t)permits : 0ULL);
                if (c[kRcDenied]) pd = wave_sum64(pd_mine ? (uint64_t)permits : 0ULL);
            }
        }
        if (lane == lead) {
            unsigned long long* cell = s_cell + r * kTcCols;
            atomicAdd(cell + kTcRequests, (unsigned long long)__popcll(m));
#pragma unroll
            for (uint32_t k = 0; k < kRcClasses; ++k)
                if (c[k]) atomicAdd(cell + report_class_col(k), (unsigned long long)c[k]);
            if (n_over) atomicAdd(cell + kTcOverMax, (unsigned long long)n_over);
            if (pa) atomicAdd(cell + kTcPermitsAllowed, (unsigned long long)pa);
            if (pd) atomicAdd(cell + kTcPermitsDenied, (unsigned long long)pd);
        }
        todo &= ~m;
    }
}

// LIM / OP: the batch has a limiter / an op array (else limiter 0 / RL_OP_ACQUIRE). They are
// template parameters, and a tile's loads are unconditional (a lane past the end reads request
// n - 1 and is switched off afterwards), so that all of a tile's loads are in flight together:
// behind per-request branches they went out one load round at a time.
template <bool LIM, bool OP>
__global__ __launch_bounds__(kTallyThreads) void k_tally(TallyArgs a) {
    __shared__ unsigned long long s_cell[kTallyCells];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < kTallyCells; i += kTallyThreads) s_cell[i] = 0;
    __syncthreads();

    const uint32_t tiles = (a.n + kTallyTile - 1) / kTallyTile;      // n <= 2^31: no wrap
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t base = tile * kTallyTile;                     // < 2^31 + 2048
        uint32_t lim[kTallyPerThread], op[kTallyPerThread];
        int32_t p[kTallyPerThread];
        uint8_t al[kTallyPerThread];
        int64_t rem[kTallyPerThread];
#pragma unroll
        for (int j = 0; j < kTallyPerThread; ++j) {
            const uint32_t i = base + (uint32_t)j * kTallyThreads + tid;
            const uint32_t at = i < a.n ? i : a.n - 1;               // n > 0 (launch_tally)
            lim[j] = LIM ? a.limiter[at] : 0u;
            op[j] = OP ? a.op[at] : 0u;
            p[j] = a.permits[at];
            al[j] = a.allowed[at];
            rem[j] = a.remaining[at];
        }
#pragma unroll
        for (int j = 0; j < kTallyPerThread; ++j) {
            const bool on = base + (uint32_t)j * kTallyThreads + tid < a.n;
            const uint32_t row = report_row(lim[j], a.n_lim) & (kTallyRows - 1);
            const uint32_t cls = report_class(lim[j], a.n_lim, op[j], p[j], al[j], rem[j]);
            wave_fold(s_cell, lane, on, row, cls, report_over_max(cls, rem[j]), (uint32_t)p[j]);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < kTallyCells; i += kTallyThreads) {
        const unsigned long long v = s_cell[i];
        if (v) atomicAdd(a.out + (i / kTcCols) * kTallyWords + i % kTcCols, v);
    }
}

}  // namespace

hipError_t launch_tally(const TallyArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint32_t tiles = (a.n + kTallyTile - 1) / kTallyTile;
    const dim3 grid(persistent_grid(tiles, kTallyPerCu)), block(kTallyThreads);
    if (a.limiter && a.op) hipLaunchKernelGGL((k_tally<true, true>), grid, block, 0, s, a);
    else if (a.limiter) hipLaunchKernelGGL((k_tally<true, false>), grid, block, 0, s, a);
    else if (a.op) hipLaunchKernelGGL((k_tally<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_tally<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace rl
