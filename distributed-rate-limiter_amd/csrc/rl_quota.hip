// rl_quota.hip — batched quota queries: for (limiter, key, now) what getAvailablePermits reads
// at now, the wait until it reads maxPermits again (X-RateLimit-Reset) and, with permits, the
// retry-after wait of rl_retry.hip, from one table lookup per key (rl_quota, include/rl_engine.h).
//
// k_retry_after's shape (rl_retry.hpp): a read-only gather, no atomics, no table write; 256
// threads, a wave owns 64 queries, four lanes probe one key, the home buckets of all four steps
// load together, the limiter table sits in LDS, every lane stores its own answers (coalesced).
// Each lane runs the decision code on its own key's slot words: the peek at now, then
// retry_search for "the peek reads maxPermits" (the cache word ignored), then retry_search for
// the acquire of permits. Both searches return only a t that the exact predicate confirmed at t
// and refuted at t - 1 (DESIGN.md §4 "Quota queries").
#include "rl_retry.hpp"

#pragma clang fp contract(off)

namespace rl {

__global__ __launch_bounds__(kRetryThreads, 4) void k_quota(QuotaArgs a) {
    extern __shared__ uint64_t s_limw[];
    const DevLimiter* s_lims = (const DevLimiter*)s_limw;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t q = blockIdx.x * kRetryBlockQueries + threadIdx.x;      // this lane's query
    // ---- the request (a skipped one is still looked up: only its retry search is skipped)
    uint64_t key = 0;
    int64_t now_ns = 0;
    int32_t p = 1;
    uint32_t lim = 0;
    bool want_retry = false;
    if (q < a.n) {
        key = a.key[q];
        now_ns = a.now_ns[q];
        if (a.limiter) lim = a.limiter[q];
        if (a.permits) {
            p = a.permits[q];
            want_retry = !(a.skip && a.skip[q] != 0);
        }
    }
    limiters_to_lds(s_limw, a.lims, a.n_lim);
    __syncthreads();
    uint32_t code = kZero;                                                 // (beyond n: nothing)
    if (q < a.n) code = (lim >= a.n_lim || (want_retry && p <= 0)) ? kInvalid : kProbe;
    const uint64_t h = code == kProbe ? mix64(key) : 0;
    const uint32_t st = (code == kProbe ? lim << 2 : 0u) | code;
    const KeyState ks = wave_lookup(s_lims, a.shard_bits, h, st, lane, nullptr);
    // ---- the answers (an absent key: all zero words, which peek as a full quota)
    int64_t rem = kQuotaInvalid, reset = kQuotaInvalid, retry = kQuotaInvalid;
    if (code == kProbe) {
        const DevLimiter& L = s_lims[lim];
        const int64_t now = floor_div_ms(now_ns);
        bool bis;
        rem = peek_remaining(L, now, ks.a, ks.b, ks.c);
        reset = 0;
        if (ks.have && rem != L.max_permits) reset = retry_search(L, true, 0, now, ks.a, ks.b, ks.c, ks.x, bis);
        retry = 0;
        if (want_retry) {
            if ((int64_t)p > L.max_permits) retry = kRetryNever;           // :110-116; SW est >= 0
            else if (ks.have) retry = retry_search(L, false, p, now, ks.a, ks.b, ks.c, ks.x, bis);
        }
    }
    if (q < a.n) {
        a.remaining[q] = rem;
        a.reset_ms[q] = reset;
        if (a.retry_ms) a.retry_ms[q] = retry;
    }
}

hipError_t launch_quota(const QuotaArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint32_t grid = (a.n + kRetryBlockQueries - 1) / kRetryBlockQueries;
    const size_t lds = (size_t)(a.n_lim ? a.n_lim : 1) * sizeof(DevLimiter);
    hipLaunchKernelGGL(k_quota, dim3(grid), dim3(kRetryThreads), lds, s, a);
    return hipGetLastError();
}

}  // namespace rl
