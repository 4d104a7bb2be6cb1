// rl_keys.hip — string keys hashed on the device (rl_hash_keys_device, rl_hash_keys,
// rl_execute_batch_keys; include/rl_engine.h): key_hash[i] = rl_key_hash(key i) = mix64 of
// FNV-1a 64 over the key's bytes, for a batch given as one byte blob plus n + 1 offsets.
//
//   k_hash_keys  a workgroup of 256 lanes takes 256 consecutive keys, one per lane. Every lane
//                loads its two offsets and checks them (key_well_formed, rl_keys.hpp) before any
//                address is formed from them; a malformed key gets 0 and is counted.
//     tile path    if every key of the workgroup is well-formed, their bytes are the one
//                  contiguous span [off[first], off[last + 1]). When the 16-byte granules that
//                  span touches fit the LDS tile, the workgroup stages them with coalesced
//                  16-byte loads and every lane walks its key out of LDS in dwords.
//     direct path  otherwise (a malformed key in the workgroup, a span beyond the tile, or
//                  KeysArgs::direct) every lane reads the 16-byte granules of its own key
//                  from global memory.
//                Both paths read a granule only if it holds a byte of a well-formed key, so a
//                read never leaves the page of a valid byte, whatever the offsets hold; granules
//                are aligned by address, so the blob's own alignment does not matter. A lane
//                makes exactly len <= kKeyMaxBytes byte steps. No floating point; the 64-bit
//                multiply by 2^40 + 0x1b3 is a 32 x 32 -> 64 multiply, a 32-bit multiply-add
//                and a shift (fnv_step).
#include "rl_kcommon.hpp"
#include "rl_keys.hpp"

namespace rl {

namespace {

constexpr int kKeysThreads = 256;
constexpr uint32_t kKeysTileBytes = 16384;               // LDS tile: 64 B per key on average
constexpr uint32_t kKeysTileGranules = kKeysTileBytes / 16;

// h = (h ^ c) * kFnvPrime mod 2^64, with kFnvPrime = 2^40 + 0x1b3.
__device__ inline uint64_t fnv_step(uint64_t h, uint32_t c) {
    const uint32_t lo = (uint32_t)h ^ c, hi = (uint32_t)(h >> 32);
    const uint64_t m = (uint64_t)lo * 0x1b3u;
    const uint32_t mh = (uint32_t)(m >> 32) + hi * 0x1b3u + (lo << 8);
    return (uint64_t)mh << 32 | (uint32_t)m;
}

// The bytes b of `word` (memory order: byte 0 is the lowest) with lo <= b < hi.
__device__ inline uint64_t eat_dword(uint64_t h, uint32_t word, int32_t lo, int32_t hi) {
    if (lo <= 0 && hi >= 4) {
        h = fnv_step(h, word & 0xffu);
        h = fnv_step(h, (word >> 8) & 0xffu);
        h = fnv_step(h, (word >> 16) & 0xffu);
        h = fnv_step(h, word >> 24);
    } else {
#pragma unroll
        for (int32_t b = 0; b < 4; ++b)
            if (b >= lo && b < hi) h = fnv_step(h, (word >> (8 * b)) & 0xffu);
    }
    return h;
}

__global__ __launch_bounds__(kKeysThreads) void k_hash_keys(KeysArgs a) {
    __shared__ uint4 tile[kKeysTileGranules];
    const uint32_t tid = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * kKeysThreads;
    const uint64_t i = first + tid;
    const bool in = i < a.n;
    RL_GLOBAL const uint64_t* off = as_global(a.off);

    // this lane's key: [o0, o0 + len) of the blob, checked before anything is derived from it
    uint64_t o0 = 0;
    uint32_t len = 0;
    bool ok = false;
    if (in) {
        const uint64_t p0 = off[i] - a.bias, p1 = off[i + 1] - a.bias;
        ok = key_well_formed(p0, p1, a.bytes_len);
        if (ok) { o0 = p0; len = (uint32_t)(p1 - p0); }
    }
    const uint64_t bad = __ballot(in && !ok);
    if (bad && (tid & 63) == 0)
        __hip_atomic_fetch_add(as_global(a.hdr), (unsigned long long)__popcll(bad), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    if (i == 0) as_global(a.hdr)[1] = a.n;

    // granules are 16-byte aligned ADDRESSES: positions count from the aligned address below the blob
    const uint32_t mis = (uint32_t)((uintptr_t)a.bytes & 15u);
    RL_GLOBAL const uint4* gran = (RL_GLOBAL const uint4*)((uintptr_t)a.bytes - mis);

    // workgroup-uniform: all keys well-formed -> their bytes are one span [s0, s1)
    const bool all_ok = __syncthreads_and(!in || ok) != 0;
    bool use_tile = false;
    uint64_t g0 = 0;                                     // the span's first granule
    uint32_t ng = 0;                                     // granules the span touches
    if (all_ok && !a.direct) {
        const uint64_t last = a.n - first < (uint64_t)kKeysThreads ? a.n : first + kKeysThreads;
        const uint64_t s0 = off[first] - a.bias, s1 = off[last] - a.bias;   // (checked above, as o0 / o1)
        if (s1 > s0) {
            g0 = (mis + s0) >> 4;
            const uint64_t g = ((mis + s1 - 1) >> 4) - g0 + 1;
            if (g <= kKeysTileGranules) { use_tile = true; ng = (uint32_t)g; }
        }
    }

    uint64_t h = kFnvOffset;
    if (use_tile) {
        for (uint32_t j = tid; j < ng; j += kKeysThreads) tile[j] = gran[g0 + j];
        __syncthreads();
        if (len) {
            const uint32_t* w = (const uint32_t*)tile;
            const uint32_t q = (uint32_t)(mis + o0 - (g0 << 4));     // the key's first byte in the tile
            const uint32_t d1 = (q + len - 1) >> 2;
            for (uint32_t d = q >> 2; d <= d1; ++d)
                h = eat_dword(h, w[d], (int32_t)q - (int32_t)(4 * d), (int32_t)(q + len) - (int32_t)(4 * d));
        }
    } else if (len) {
        const uint64_t p = mis + o0;
        const uint32_t skip = (uint32_t)(p & 15u);       // the key's first byte in its first granule
        const uint32_t n16 = (skip + len + 15) >> 4;     // granules that hold a byte of this key
        RL_GLOBAL const uint4* gp = gran + (p >> 4);
        int32_t lo = (int32_t)skip, hi = (int32_t)(skip + len);
        for (uint32_t g = 0; g < n16; ++g, lo -= 16, hi -= 16) {
            const uint4 v = gp[g];
            h = eat_dword(h, v.x, lo, hi);
            h = eat_dword(h, v.y, lo - 4, hi - 4);
            h = eat_dword(h, v.z, lo - 8, hi - 8);
            h = eat_dword(h, v.w, lo - 12, hi - 12);
        }
    }
    if (in) as_global(a.out)[i] = ok ? mix64(h) : 0ULL;
}

}  // namespace

hipError_t launch_hash_keys(const KeysArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)((a.n + kKeysThreads - 1) / kKeysThreads);
    hipLaunchKernelGGL(k_hash_keys, dim3(grid), dim3(kKeysThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace rl
