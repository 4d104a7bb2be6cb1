// rl_digest.hip — per-bucket fingerprints of one limiter's live state (rl_limiter_digest,
// rl_limiter_digest_device, include/rl_engine.h): for every bucket of the table (the top
// bucket_bits of the region index) the count, the wrapping sum and the xor of a 64-bit hash of
// every entry that is live at `now`. The entries are the Redis keys live_buckets (rl_table.hpp)
// finds in a slot, the ones rl_export_state emits, and on request the local-cache words that
// reject at `now`; the hash covers the key's tag and the entry's logical fields, not the stored
// words, so where a key sits, tombstones and the table's size do not matter.
//
//   k_digest   one read-only pass over the limiter's slots. The work unit is a region (256
//              consecutive slots = 8 KB, always inside one bucket): a wave issues the region's
//              four 64-slot loads (and cache-word loads) together and then hashes what is live.
//              Every wave owns a CONTIGUOUS span of regions (not a grid-strided one), so it
//              crosses few bucket boundaries: lanes keep their own (entries, sum, xr) while the
//              bucket stays the same; at a boundary, and at the end of the span, the wave
//              reduces over its 64 lanes (DPP) and lane 0 folds the three words into
//              out[bucket] with two 64-bit atomic adds and one atomic xor, or with plain stores
//              when the wave's run covered the whole bucket (nobody else writes it then; `out`
//              is zeroed on the stream first). No per-slot atomic. Add and xor commute, so the
//              result does not depend on the grid (rl_tune "digest_per_cu").
//   k_digest_fold  for fewer than 2^kDigestFineBits buckets the pass runs at kDigestFineBits (or
//              the table's region bits) into a scratch and this kernel adds each bucket's run of
//              fine digests (buckets are prefixes of finer buckets), one wave per bucket, plain
//              stores: thousands of waves folding into a handful of addresses would serialise on
//              them (measured: one bucket on a 64 MB table 0.32 ms, 4096 buckets 0.044 ms).
#include "rl_table.hpp"

#pragma clang fp contract(off)

namespace rl {

namespace {

constexpr int kDigestThreads = 256;
constexpr int kDigestWaves = kDigestThreads / 64;
constexpr uint32_t kDigestSteps = kRegionSlots / 64;      // 64-slot loads per region

__device__ inline uint64_t rotl64(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }

// H(entry) of include/rl_engine.h: four 64-bit multiplies.
__device__ inline uint64_t entry_hash(uint64_t tag, uint64_t kind, uint64_t f1, uint64_t f2, uint64_t f3) {
    uint64_t u = tag + kind;
    u = (u ^ f1) * kDigestC1;
    u = (u ^ rotl64(f2, 23)) * kDigestC2;
    u ^= rotl64(f3, 47);
    return mix64(u);
}

struct DigestAcc {
    uint64_t n = 0, sum = 0, xr = 0;
    __device__ inline void add(uint64_t h) { n += 1; sum += h; xr ^= h; }
};

// The entries of one slot at `now` (a free slot has none: no live bucket, no cache word).
__device__ inline void digest_slot(DigestAcc& acc, const DevLimiter& L, const Slot& v, uint64_t x, int64_t now) {
    const LiveBuckets lb = live_buckets(L, v, now);
    if (L.algo == kAlgoTB) {
        if (lb.n) acc.add(entry_hash(v.tag, kDigestKTb, v.a, (uint64_t)lb.start[0], (uint64_t)lb.deadline[0]));
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 2; ++j)
            if (j < lb.n)
                acc.add(entry_hash(v.tag, kDigestKSw, (uint64_t)lb.start[j], (uint64_t)lb.count[j],
                                   (uint64_t)lb.deadline[j]));
    }
    if (x != 0 && now < (int64_t)x) acc.add(entry_hash(v.tag, kDigestKCache, x, 0, 0));
}

// The wave's sums of one run of regions into out[bucket]; every lane of the wave takes part.
__device__ inline void digest_flush(RL_GLOBAL BucketDigest* o, const DigestAcc& acc, bool whole, uint32_t lane) {
    const uint64_t n = wave_reduce_dpp(acc.n, [](uint64_t p, uint64_t q) { return p + q; });
    const uint64_t sum = wave_reduce_dpp(acc.sum, [](uint64_t p, uint64_t q) { return p + q; });
    const uint64_t xr = wave_reduce_dpp(acc.xr, [](uint64_t p, uint64_t q) { return p ^ q; });
    if (lane != 0) return;
    if (whole) {                                   // the run was the whole bucket: no other writer
        o->entries = n; o->sum = sum; o->xr = xr;
    } else if (n) {
        __hip_atomic_fetch_add(&o->entries, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&o->sum, (unsigned long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_xor(&o->xr, (unsigned long long)xr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kDigestThreads) void k_digest(DigestArgs a) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    // this wave's span of regions [r, r_end) (wave-uniform, so is everything derived from it)
    const uint64_t n_waves = (uint64_t)gridDim.x * kDigestWaves;
    const uint64_t per = (a.n_regions + n_waves - 1) / n_waves;
    uint64_t r = ((uint64_t)blockIdx.x * kDigestWaves + wid) * per;
    if (r >= a.n_regions) return;
    const uint64_t r_end = r + per < a.n_regions ? r + per : a.n_regions;
    const uint32_t shift = (uint32_t)a.L.region_bits - a.bucket_bits;      // log2(regions per bucket)
    RL_GLOBAL const Slot* tab = as_global(a.tab);
    RL_GLOBAL const uint64_t* xtab =
        (a.with_cache && a.L.cache_table) ? as_global((const uint64_t*)a.L.cache_table) : nullptr;
    RL_GLOBAL BucketDigest* out = as_global(a.out);
    DigestAcc acc;
    uint64_t run0 = r;                             // first region of the run in `acc`
    for (; r < r_end; ++r) {
        Slot v[kDigestSteps];
        uint64_t x[kDigestSteps];
        const uint64_t s0 = r * kRegionSlots + lane;
#pragma unroll
        for (uint32_t j = 0; j < kDigestSteps; ++j) {
            v[j] = tab[s0 + 64 * j];
            x[j] = xtab ? xtab[s0 + 64 * j] : 0;
        }
#pragma unroll
        for (uint32_t j = 0; j < kDigestSteps; ++j) digest_slot(acc, a.L, v[j], x[j], a.now);
        const uint64_t b = r >> shift;
        if (r + 1 == r_end || ((r + 1) >> shift) != b) {
            const bool whole = run0 == (b << shift) && r + 1 == ((b + 1) << shift);
            digest_flush(out + b, acc, whole, lane);
            acc = DigestAcc{};
            run0 = r + 1;
        }
    }
}

// out[b] = the fine digests [b << d, (b + 1) << d) combined; one wave per bucket.
__global__ __launch_bounds__(64) void k_digest_fold(const BucketDigest* __restrict__ fine, uint32_t d,
                                                    BucketDigest* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    const uint64_t b = blockIdx.x, m = 1ULL << d;
    DigestAcc acc;
    for (uint64_t i = lane; i < m; i += 64) {
        const BucketDigest f = fine[(b << d) + i];
        acc.n += f.entries; acc.sum += f.sum; acc.xr ^= f.xr;
    }
    digest_flush(as_global(out + b), acc, true, lane);
}

}  // namespace

hipError_t launch_digest_fold(const BucketDigest* fine, uint32_t fine_bits, BucketDigest* out,
                              uint32_t bucket_bits, hipStream_t s) {
    hipLaunchKernelGGL(k_digest_fold, dim3(1u << bucket_bits), dim3(64), 0, s, fine, fine_bits - bucket_bits, out);
    return hipGetLastError();
}

hipError_t launch_digest(const DigestArgs& a, hipStream_t s) {
    if (a.n_regions == 0) return hipSuccess;
    const uint64_t blocks = (a.n_regions + kDigestWaves - 1) / kDigestWaves;
    const uint32_t grid = persistent_grid((uint32_t)std::min<uint64_t>(blocks, 1u << 30),
                                          a.per_cu ? a.per_cu : kDigestPerCu);
    hipLaunchKernelGGL(k_digest, dim3(grid), dim3(kDigestThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace rl
