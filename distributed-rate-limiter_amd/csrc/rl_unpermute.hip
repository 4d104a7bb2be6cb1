// rl_unpermute.hip — the packed results back to arrival order (k_unpermute, its split form,
// the two-pass batches' k_unpermute_mid) and the all-invalid fill, for gfx950.
#include "rl_kcommon.hpp"

#pragma clang fp contract(off)

namespace rl {

// A packed result decoded to the caller's (allowed, remaining) of request i.
template <bool NT, class Res>
__device__ __forceinline__ void store_decision(const UnpermArgs& a, uint32_t i, Res v) {
    st<NT>(a.allowed + i, (uint8_t)(v & 1u));
    st<NT>(a.remaining + i, (int64_t)(v >> 1) - kResBias);
}

// Rare (TB balances below -3 after time regression): the gather decoded the escape code as
// (allowed 1, remaining -3); rewrite those results from the side array. Same tiles, same
// thread t per element as the kernel's stores, so the rewrite follows the first store.
template <class Res>
__device__ __forceinline__ void fix_escapes(const UnpermArgs& a, uint32_t t) {
    if (!a.ctl || a.ctl->n_esc == 0) return;
    const Res* rf = (const Res*)a.res_final;
    for (uint32_t it = 0;; ++it) {
        const uint32_t tile = tile_at(it, a.n_tiles);
        if (tile >= a.n_tiles) break;
        for (int r = 0; r < kTileItems; ++r) {
            const uint32_t i = tile * (uint32_t)kTile + (uint32_t)r * kTileThreads + t;
            if (i >= a.n) break;
            uint32_t j = a.pos0[i];
            if (a.pos1_final && j < a.ctl->n_normal) j = a.pos1_final[j];
            if ((uint64_t)rf[j] == kResEscape) {
                a.allowed[i] = 0;
                a.remaining[i] = a.ext[j];
            }
        }
    }
}

template <class Res>
__global__ __launch_bounds__(kTileThreads) void k_unpermute(UnpermArgs a) {
  const uint32_t t = threadIdx.x;
  const Res* __restrict__ res = (const Res*)a.res;
  const uint32_t* __restrict__ pos0 = a.pos0;
  const uint32_t* __restrict__ pos1 = a.pos1;
  constexpr int B = 8;                         // rounds per batch (loads issued together)
  constexpr int NB = kTileItems / B;
  const bool simple = pos1 || a.tokens_out || (RL_ABLATION(a) & kAblNoGather);
  // two-pass batches: mid (res) holds the normal records' results in pass-0 order, res_hi
  // the routed records' results at their own (pass-0) positions >= n_normal
  const Res* __restrict__ res_hi = (const Res*)a.res_hi;
  const uint32_t nn = res_hi ? a.ctl->n_normal : 0u;
  for (uint32_t it = 0;; ++it) {
    const uint32_t tile = tile_at(it, a.n_tiles);
    if (tile >= a.n_tiles) break;
    const uint32_t tbase = tile * (uint32_t)kTile + t;
    if (!simple && tile * (uint64_t)kTile + kTile <= a.n) {
        // Full tile, one result array: software-pipelined so that every wait is for loads
        // issued a batch earlier and never directly behind the previous batch's stores
        // (vmcnt retires loads and stores in issue order).
        uint32_t pE[B], pO[B];
        Res vE[B], vO[B];
        auto load = [&](uint32_t (&p)[B], int b) {
#pragma unroll
            for (int k = 0; k < B; ++k) p[k] = ld<kNtUn>(pos0 + tbase + (uint32_t)(b * B + k) * kTileThreads);
        };
        auto gather = [&](Res (&v)[B], const uint32_t (&p)[B]) {
#pragma unroll
            for (int k = 0; k < B; ++k) v[k] = (res_hi && p[k] >= nn ? res_hi : res)[p[k]];
        };
        auto store = [&](const Res (&v)[B], int b) {
#pragma unroll
            for (int k = 0; k < B; ++k)
                store_decision<kNtUn>(a, tbase + (uint32_t)(b * B + k) * kTileThreads, v[k]);
        };
        load(pE, 0);
        for (int b = 0; b < NB; b += 2) {
            gather(vE, pE);
            load(pO, b + 1);
            if (b > 0) store(vO, b - 1);
            gather(vO, pO);
            load(pE, (b + 2) % NB);                 // unconditional (last one unused)
            store(vE, b);
        }
        store(vO, NB - 1);
        continue;
    }
    for (int r0 = 0; r0 < kTileItems; r0 += B) {
        uint32_t p[B];
        Res v[B];
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const uint32_t i = tile * (uint32_t)kTile + (uint32_t)(r0 + k) * kTileThreads + t;
            p[k] = pos0[i < a.n ? i : 0];
        }
        if (pos1) {
            // pass 1 moved the normal records only; routed ones kept their pass-0 position
            const uint32_t nn = a.ctl->n_normal;
#pragma unroll
            for (int k = 0; k < B; ++k) p[k] = p[k] < nn ? pos1[p[k]] : p[k];
        }
        if (RL_ABLATION(a) & kAblNoGather) {
#pragma unroll
            for (int k = 0; k < B; ++k) v[k] = (Res)p[k];
        } else {
#pragma unroll
            for (int k = 0; k < B; ++k) v[k] = (res_hi && p[k] >= nn ? res_hi : res)[p[k]];
        }
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const uint32_t i = tile * (uint32_t)kTile + (uint32_t)(r0 + k) * kTileThreads + t;
            if (i < a.n) {
                store_decision<false>(a, i, v[k]);
                if (a.tokens_out) a.tokens_out[i] = a.tok ? a.tok[p[k]] : __builtin_nan("");
            }
        }
    }
  }
  fix_escapes<Res>(a, t);
}

// Split unpermute (rl_tune unpermute_split): the position reads and result gathers in loader
// waves (threads kTileThreads..), the decision stores in storer waves, one round apart through
// LDS, so that no wait for a gather sits behind the acks of earlier stores (one vmcnt for both
// on gfx950). Loaders keep kUnPosDepth rounds of positions and kUnGatherDepth rounds of
// gathers in flight. One-array batches only (no pos1 pass, no tokens): k_unpermute otherwise.
constexpr int kUnPosDepth = 8, kUnGatherDepth = 4;
template <class Res>
__global__ __launch_bounds__(2 * kTileThreads) void k_unpermute_split(UnpermArgs a) {
    __shared__ Res stage[2][kTileThreads];
    const uint32_t t = threadIdx.x;
    const bool loader = t >= (uint32_t)kTileThreads;          // (wave-uniform)
    const uint32_t lt = loader ? t - (uint32_t)kTileThreads : t;
    const Res* __restrict__ res = (const Res*)a.res;
    const Res* __restrict__ res_hi = (const Res*)a.res_hi;
    const uint32_t nn = res_hi ? a.ctl->n_normal : 0u;
    const uint32_t last = a.n - 1;
    for (uint32_t it = 0;; ++it) {
        const uint32_t tile = tile_at(it, a.n_tiles);
        if (tile >= a.n_tiles) break;
        const uint32_t tbase = tile * (uint32_t)kTile + lt;
        __syncthreads();                                      // last tile's stage readers are done
        if (loader) {
            uint32_t P[kUnPosDepth];
            Res V[kUnGatherDepth];
            auto pos_of = [&](int r) { return ld<kNtUn>(a.pos0 + min(tbase + (uint32_t)r * kTileThreads, last)); };
            auto gather = [&](uint32_t p) { return (res_hi && p >= nn ? res_hi : res)[p]; };
#pragma unroll
            for (int k = 0; k < kUnPosDepth; ++k) P[k] = pos_of(k);
#pragma unroll
            for (int k = 0; k < kUnGatherDepth; ++k) {
                V[k] = gather(P[k]);
                P[k] = pos_of(k + kUnPosDepth);
            }
            // round r: stage round r's results; gather round r + G (its position, slot
            // (r + G) % D, arrived); reload that slot with round r + G + D
            for (int r0 = 0; r0 < kTileItems; r0 += kUnPosDepth) {
#pragma unroll
                for (int k = 0; k < kUnPosDepth; ++k) {
                    const int r = r0 + k;
                    stage[r & 1][lt] = V[k % kUnGatherDepth];
                    V[k % kUnGatherDepth] = gather(P[(k + kUnGatherDepth) % kUnPosDepth]);
                    P[(k + kUnGatherDepth) % kUnPosDepth] = pos_of(r + kUnGatherDepth + kUnPosDepth);
                    __syncthreads();
                }
            }
        } else {
            for (int r = 0; r < kTileItems; ++r) {
                __syncthreads();
                const Res v = stage[r & 1][lt];
                const uint32_t i = tbase + (uint32_t)r * kTileThreads;
                if (i < a.n) store_decision<kNtUn>(a, i, v);
            }
        }
    }
    if (!loader) fix_escapes<Res>(a, t);         // by the thread that stored the result
}

// Two-pass batches: undo the high-digit pass first. mid[j] = res[pos1[j]] for j in
// pass-0 order: pos1 is read in order and, since pass 0 left the records sorted by low
// digit, consecutive j fall into one low-digit run whose elements go to the 2^d1
// high-digit bins in order — the gather walks 2^d1 sequential streams instead of the
// whole result array. k_unpermute then gathers mid[pos0[i]] (2^d0 streams). Two
// local gathers replace the composed res[pos1[pos0[i]]], which hit a random line of a
// 1 GB index and of the result array per request.
// Routed records (pass-0 positions >= ctl->n_normal) skipped pass 1: k_unpermute reads
// their results in place (UnpermArgs::res_hi), so mid covers the normal records only.
template <class Res>
__global__ __launch_bounds__(256) void k_unpermute_mid(const uint32_t* __restrict__ pos1,
                                                       const Res* __restrict__ res,
                                                       Res* __restrict__ mid, uint32_t n,
                                                       const BatchCtl* __restrict__ ctl, uint32_t xcd) {
    constexpr int B = 8;
    // consecutive blocks of j on one XCD: a pass-0 bin's 2^d1 result streams are then read
    // through one L2 instead of being fetched into all eight
    const uint32_t base = (xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x) * (256u * B) + threadIdx.x;
    n = min(n, ctl->n_normal);
    if (base >= n) return;
    uint32_t p[B];
#pragma unroll
    for (int k = 0; k < B; ++k) {
        const uint32_t j = base + (uint32_t)k * 256u;
        p[k] = pos1[j < n ? j : base];
    }
    Res v[B];
#pragma unroll
    for (int k = 0; k < B; ++k) v[k] = res[p[k]];
#pragma unroll
    for (int k = 0; k < B; ++k) {
        const uint32_t j = base + (uint32_t)k * 256u;
        if (j < n) mid[j] = v[k];
    }
}

__global__ void k_fill_invalid(uint8_t* allowed, int64_t* remaining, double* tok, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        allowed[i] = 0;
        remaining[i] = kRemInvalid;
        if (tok) tok[i] = __builtin_nan("");
    }
}

// f(Res{}) with the packed result type of res_bytes (1, 2, 8; else 4).
template <class F>
static void with_res_type(int res_bytes, F f) {
    if (res_bytes == 8) f(uint64_t{});
    else if (res_bytes == 1) f(uint8_t{});
    else if (res_bytes == 2) f(uint16_t{});
    else f(uint32_t{});
}

hipError_t launch_unpermute(const UnpermArgs& a_in, int res_bytes, hipStream_t s) {
    UnpermArgs a = a_in;
    a.res_final = a.res;
    a.pos1_final = a.pos1;
    const bool mid = a.pos1 && a.mid && !a.tokens_out && a.n;   // two-pass: undo pass 1, then pass 0
    const dim3 g(persistent_grid(a.n_tiles, a.per_cu ? a.per_cu : 1));
    with_res_type(res_bytes, [&](auto r) {
        using Res = decltype(r);
        if (mid) {
            hipLaunchKernelGGL(k_unpermute_mid<Res>, dim3((a.n + 2047) / 2048), dim3(256), 0, s, a.pos1,
                               (const Res*)a.res, (Res*)a.mid, a.n, a.ctl, a.mid_xcd);
            a.res_hi = a.res;
            a.res = a.mid;
            a.pos1 = nullptr;
        }
        if (a.split && !a.pos1 && !a.tokens_out && !RL_ABLATION(a))
            hipLaunchKernelGGL(k_unpermute_split<Res>, g, dim3(2 * kTileThreads), 0, s, a);
        else
            hipLaunchKernelGGL(k_unpermute<Res>, g, dim3(kTileThreads), 0, s, a);
    });
    return hipGetLastError();
}

hipError_t launch_fill_invalid(uint8_t* allowed, int64_t* remaining, double* tok, uint32_t n,
                               hipStream_t s) {
    hipLaunchKernelGGL(k_fill_invalid, dim3((n + 255) / 256), dim3(256), 0, s, allowed,
                       remaining, tok, n);
    return hipGetLastError();
}

}  // namespace rl
