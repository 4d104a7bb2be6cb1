// rl_retry.hip — batched retry-after queries: for (limiter, key, permits, now) the first
// millisecond t >= now at which tryAcquire(key, permits) would be allowed on the key's state
// as it stands, without applying it (rl_retry_after, include/rl_engine.h).
//
// A read-only gather: no partition, no region image, no atomics, no table write. Four lanes
// look one key up (16 keys per wave at a time) with the quad probe of rl_table.hpp. A wave takes
// 64 queries, so it does four such steps with their home-bucket loads in flight together; the
// slots then go to the lanes that own the queries, and every lane searches for its own answer
// and stores it. The limiter table sits in LDS (the only LDS use). The lookup and the search
// are rl_retry.hpp's (wave_lookup, retry_search), shared with the quota lookup (rl_quota.hip).
#include "rl_retry.hpp"

#pragma clang fp contract(off)

namespace rl {

// A wave answers 64 consecutive queries, lane i owning query i: it reads the request and, at
// the end, searches and stores the answer (coalesced, every lane busy in the search). In
// between the wave looks the 64 keys up (wave_lookup, rl_retry.hpp). The dependent global loads
// are two deep (the request arrays, then the home buckets of all four steps at once); the
// limiter table is read from LDS, where the workgroup puts it while the request loads are in
// flight.
__global__ __launch_bounds__(kRetryThreads, 4) void k_retry_after(RetryArgs a) {
    extern __shared__ uint64_t s_limw[];
    const DevLimiter* s_lims = (const DevLimiter*)s_limw;
    const uint32_t lane = threadIdx.x & 63;
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
    limiters_to_lds(s_limw, a.lims, a.n_lim);
    __syncthreads();
    uint32_t code = kZero;
    if (q < a.n && sk == 0) {
        if (lim >= a.n_lim || p <= 0) code = kInvalid;
        else if ((int64_t)p > s_lims[lim].max_permits) code = kNever;   // :110-116; SW est >= 0
        else code = kProbe;
    }
    const uint64_t h = code == kProbe ? mix64(key) : 0;
    const uint32_t st = (code == kProbe ? lim << 2 : 0u) | code;
#ifdef RL_RETRY_COUNT
    unsigned long long* const probed = a.dbg ? a.dbg + 2 : nullptr;
#else
    unsigned long long* const probed = nullptr;
#endif
    const KeyState ks = wave_lookup(s_lims, a.shard_bits, h, st, lane, probed);
    // ---- the answer (skipped 0, invalid, never; an absent key grants any p <= max at once: 0)
    int64_t out = code == kInvalid ? kRetryInvalid : code == kNever ? kRetryNever : 0;
    if (code == kProbe && ks.have) {
        bool bis;
        out = retry_search(s_lims[lim], false, p, floor_div_ms(now_ns), ks.a, ks.b, ks.c, ks.x, bis);
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
