// rl_group.hip — local grouping of a two-pass batch: each normal pass-0 bin's records grouped
// by region inside the bin's own range of the final record array, for gfx950.
#include "rl_kcommon.hpp"

#pragma clang fp contract(off)

namespace rl {

// Two-pass batches. Pass 0 partitions by the HIGH dh bits of the region id (bin = region >>
// s0; routed hot regions to bins of their own), so a normal pass-0 bin holds the records of
// 2^s0 consecutive regions in arrival order. The bins are then grouped by region inside their
// own ranges of the final array. A bin is cut into tiles of group_tile_recs records (8192):
//   k_gtiles  tiles per bin (scan) and each tile's bin;
//   k_gcount  one wave per tile: its records per region (wave-private LDS counters);
//   k_gscan   one workgroup per bin: per region, the prefix over the bin's tiles, then the
//             regions' starts (region-major, then tile: stable) -> each tile's cursors and
//             the regions' bounds (rstart / rend: the old k_bin_bounds searches are gone);
//   k_gplace  one wave per tile: rank inside each 64-record round by ballot match, place at
//             the tile's own cursors (no barrier), pos_out[j] = final position.
// A tile's output lands in the bin's window (a few hundred KB) within microseconds, so the
// scattered 16-B record stores complete their sectors while the lines are still in L2 (the
// global second pass spread every bin's runs over the whole batch and left half-written
// sectors: write amplification 1.57x). Tiles rather than one workgroup per bin: the largest
// bins hold ~8x the mean (sw_zipf: 230K records against 30K), and one workgroup per bin made
// the largest set the stage (2.0 ms). pos_out keeps the unpermute's two gathers local.
constexpr int kGroupThreads = 256;
constexpr int kGroupWaves = kGroupThreads / 64;
constexpr int kGroupDepth = 8;                       // rounds of records in flight per wave

__global__ __launch_bounds__(1024) void k_gtiles(GroupArgs a) {
    __shared__ uint32_t tmp[16];
    const uint32_t t = threadIdx.x, nb = a.n_bins0, T = a.tile_recs;
    const uint32_t per = (nb + 1023) / 1024;
    const uint32_t b0 = min(t * per, nb), b1 = min(b0 + per, nb);
    const uint32_t S = a.seg_start ? a.n_segs : 1u;
    // (segmented: a bin's runs in segment order, tiles never crossing a run)
    auto run_of = [&](uint32_t b, uint32_t s, uint32_t& st, uint32_t& c) {
        if (a.seg_start) { st = a.seg_start[b * S + s]; c = a.seg_cnt[b * S + s]; }
        else { st = a.bin_base[b]; c = a.bin_total[b]; }
    };
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; ++b)
        for (uint32_t s = 0; s < S; ++s) {
            uint32_t st, c;
            run_of(b, s, st, c);
            sum += (c + T - 1) / T;
        }
    uint32_t tot;
    uint32_t base = block_exclusive_scan<1024>(sum, tmp, &tot);
    for (uint32_t b = b0; b < b1; ++b) {
        a.tile_base[b] = min(base, a.max_tiles);
        for (uint32_t s = 0; s < S; ++s) {
            uint32_t st, c;
            run_of(b, s, st, c);
            const uint32_t nt = (c + T - 1) / T;
            for (uint32_t j = 0; j < nt && base + j < a.max_tiles; ++j) {
                a.tile_bin[base + j] = b;
                if (a.seg_start) {
                    a.tile_beg[base + j] = st + j * T;
                    a.tile_end[base + j] = st + min((j + 1) * T, c);
                }
            }
            base += nt;
        }
    }
    if (t == 0) a.tile_base[nb] = min(tot, a.max_tiles);
}

// (tile t of the batch: bin, first record, end)
__device__ inline void group_tile(const GroupArgs& a, uint32_t t, uint32_t& b, uint32_t& beg,
                                  uint32_t& end) {
    b = a.tile_bin[t];
    if (a.seg_start) {
        beg = a.tile_beg[t];
        end = a.tile_end[t];
        return;
    }
    const uint32_t j = t - a.tile_base[b];
    const uint32_t bb = a.bin_base[b], be = bb + a.bin_total[b];
    beg = bb + j * a.tile_recs;
    end = min(beg + a.tile_recs, be);
}

// This lane's records of the kGroupDepth rounds from i0 (past the tile's end: its last record).
template <class Rec>
__device__ __forceinline__ void load_rounds(Rec (&r)[kGroupDepth], const Rec* __restrict__ in,
                                            uint32_t i0, uint32_t end, uint32_t lane) {
#pragma unroll
    for (int k = 0; k < kGroupDepth; ++k) {
        const uint32_t i = i0 + (uint32_t)k * 64 + lane;
        r[k] = ld_rec<kNtRgRec>(in + (i < end ? i : end - 1));
    }
}

template <class Codec>
__global__ __launch_bounds__(kGroupThreads) void k_gcount(GroupArgs a) {
    using Rec = typename Codec::Rec;
    extern __shared__ uint32_t gl[];                 // [waves][2^s0]
    __shared__ LimLds L;
    load_lim_lds(L, a.lims, a.n_lim);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t nsub = 1u << a.sub_bits, smask = nsub - 1u;
    uint32_t* cw = gl + wid * nsub;
    const Rec* __restrict__ in = (const Rec*)a.rec_in;
    const uint32_t n_t = a.tile_base[a.n_bins0];
    for (uint32_t t = blockIdx.x * kGroupWaves + wid; t < n_t; t += gridDim.x * kGroupWaves) {
        uint32_t b, beg, end;
        group_tile(a, t, b, beg, end);
        for (uint32_t k = lane; k < nsub; k += 64) cw[k] = 0;
        wave_fence();
        for (uint32_t i0 = beg; i0 < end; i0 += 64 * kGroupDepth) {
            Rec r[kGroupDepth];
            load_rounds(r, in, i0, end, lane);
#pragma unroll
            for (int k = 0; k < kGroupDepth; ++k)
                if (i0 + (uint32_t)k * 64 + lane < end)
                    atomicAdd(&cw[region_of_rec<Codec>(L, r[k], a.shard_bits) & smask], 1u);
        }
        wave_fence();
        uint32_t* dst = a.tcount + (size_t)t * nsub;
        for (uint32_t k = lane; k < nsub; k += 64) dst[k] = cw[k];
        wave_fence();
    }
}

__global__ __launch_bounds__(kGroupThreads) void k_gscan(GroupArgs a) {
    extern __shared__ uint32_t tot[];                // [2^s0] the regions' record counts
    __shared__ uint32_t tmp[kGroupWaves];
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    const uint32_t nsub = 1u << a.sub_bits;
    const uint32_t t0 = a.tile_base[b], t1 = a.tile_base[b + 1 <= a.n_bins0 ? b + 1 : b];
    // per region: the prefix over the bin's tiles (in place)
    for (uint32_t k = t; k < nsub; k += kGroupThreads) {
        uint32_t run = 0;
        for (uint32_t j = t0; j < t1; ++j) {
            uint32_t* c = a.tcount + (size_t)j * nsub + k;
            const uint32_t v = *c;
            *c = run;
            run += v;
        }
        tot[k] = run;
    }
    __syncthreads();
    // the regions' starts: a contiguous chunk of regions per thread, one block scan
    const uint32_t per = (nsub + kGroupThreads - 1) / kGroupThreads;
    const uint32_t k0 = min(t * per, nsub), k1 = min(k0 + per, nsub);
    uint32_t sum = 0;
    for (uint32_t k = k0; k < k1; ++k) sum += tot[k];
    uint32_t run = a.bin_base[b] + block_exclusive_scan<kGroupThreads>(sum, tmp, nullptr);
    const uint32_t g0 = b << a.sub_bits;
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t c = tot[k];
        tot[k] = run;
        if (g0 + k < a.n_regions) {
            a.rstart[g0 + k] = run;
            a.rend[g0 + k] = run + c;
        }
        run += c;
    }
    __syncthreads();
    for (uint32_t k = t; k < nsub; k += kGroupThreads) {
        const uint32_t st = tot[k];
        for (uint32_t j = t0; j < t1; ++j) a.tcount[(size_t)j * nsub + k] += st;
    }
}

template <class Codec>
__global__ __launch_bounds__(kGroupThreads) void k_gplace(GroupArgs a) {
    using Rec = typename Codec::Rec;
    extern __shared__ uint32_t gl[];                 // [waves][2^s0]: the tile's cursors
    __shared__ LimLds L;
    load_lim_lds(L, a.lims, a.n_lim);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t nsub = 1u << a.sub_bits, smask = nsub - 1u;
    uint32_t* cw = gl + wid * nsub;
    const Rec* __restrict__ in = (const Rec*)a.rec_in;
    Rec* __restrict__ out = (Rec*)a.rec_out;
    const uint32_t n_t = a.tile_base[a.n_bins0];
    // Every lane loads and stores in every round (past the tile's end: the last record again,
    // stored to the padding past the batch), and the next rounds' records are loaded before
    // this round's stores: with no memory operation under a branch the wait-count pass counts
    // statically, so waiting for a round's records does not drain the stores issued before it
    // (one vmcnt for both on gfx950).
    const uint32_t pad = a.pad + lane;
    for (uint32_t t = blockIdx.x * kGroupWaves + wid; t < n_t; t += gridDim.x * kGroupWaves) {
        uint32_t b, beg, end;
        group_tile(a, t, b, beg, end);
        const uint32_t* src = a.tcount + (size_t)t * nsub;
        for (uint32_t k = lane; k < nsub; k += 64) cw[k] = src[k];
        wave_fence();
        auto place = [&](const Rec (&r)[kGroupDepth], uint32_t i0) {
#pragma unroll
            for (int k = 0; k < kGroupDepth; ++k) {
                const uint32_t i = i0 + (uint32_t)k * 64 + lane;
                const bool act = i < end;
                const uint32_t sb = act ? region_of_rec<Codec>(L, r[k], a.shard_bits) & smask : 0u;
                const uint64_t m = wave_match(sb, (int)a.sub_bits, act);
                const uint32_t lr = popc_below(m);
                const uint32_t pos = cw[sb] + lr;
                wave_fence();                            // every lane has read its cursor
                if (act && lr == 0) cw[sb] = pos + (uint32_t)__popcll(m);
                wave_fence();
                const uint32_t wp = (RL_ABLATION(a) & kAblGroupSeq) ? i : pos;
                st_rec<false>(out + (act ? wp : pad), r[k]);    // (temporal: sectors merge in L2)
                st<kNtScPos>(a.pos_out + (act ? i : pad), act ? pos : 0u);
            }
        };
        Rec ra[kGroupDepth], rb[kGroupDepth];
        load_rounds(ra, in, beg, end, lane);
        for (uint32_t i0 = beg; i0 < end; i0 += 128 * kGroupDepth) {
            load_rounds(rb, in, i0 + 64 * kGroupDepth, end, lane);
            place(ra, i0);
            if (i0 + 64 * kGroupDepth >= end) break;     // (wave-uniform)
            load_rounds(ra, in, i0 + 128 * kGroupDepth, end, lane);
            place(rb, i0 + 64 * kGroupDepth);
        }
        wave_fence();
    }
}

// k_gplace with the tile's records sorted by region in LDS first, in chunks of kGChunk: the
// global stores then go out as runs of consecutive records per region (a wave-instruction
// covers a few lines instead of 64 scattered 16-B pieces: with every record scattered,
// k_gplace ran 1.5 ms on sw_zipf, with the same stores made contiguous 0.9 ms). Each wave
// ranks its own 256 records of the chunk (4 rounds, ballot match, wave-private counts), the
// counts are scanned region-major then wave (stable), records go to their sorted slot in
// LDS, and the chunk is written out in sorted order; the tile's cursors advance per chunk.
// For bins of up to 2^kGLdsMaxSub regions (wider ones take k_gplace).
constexpr int kGPThreads = 512;
constexpr int kGPWaves = kGPThreads / 64;
constexpr uint32_t kGChunk = 2048;                   // records sorted in LDS at once
constexpr uint32_t kGLdsMaxSub = 10;
template <class Rec>
__host__ __device__ inline size_t gplace_lds_bytes(uint32_t sub_bits) {
    const size_t nsub = (size_t)1 << sub_bits;
    return kGChunk * sizeof(Rec) + kGChunk * 2 + kGPWaves * nsub * 2 + 2 * nsub * 4;
}
template <class Codec>
__global__ __launch_bounds__(kGPThreads) void k_gplace_lds(GroupArgs a) {
    using Rec = typename Codec::Rec;
    extern __shared__ uint4 glds[];
    __shared__ LimLds L;
    __shared__ uint32_t s_tmp[kGPWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const uint32_t nsub = 1u << a.sub_bits, smask = nsub - 1u;
    Rec* stg = (Rec*)glds;                            // [kGChunk] the chunk, sorted
    uint16_t* ssub = (uint16_t*)(stg + kGChunk);      // [kGChunk] their regions
    uint16_t* hist = ssub + kGChunk;                  // [waves][nsub] counts, then wave prefixes
    uint32_t* tsub = (uint32_t*)(hist + kGPWaves * nsub);   // [nsub] chunk-local region starts
    uint32_t* gcur = tsub + nsub;                     // [nsub] the tile's global cursors
    load_lim_lds(L, a.lims, a.n_lim);
    const Rec* __restrict__ in = (const Rec*)a.rec_in;
    Rec* __restrict__ out = (Rec*)a.rec_out;
    const uint32_t n_t = a.tile_base[a.n_bins0];
    const uint32_t per = (nsub + kGPThreads - 1) / kGPThreads;
    const uint32_t k0 = min(t * per, nsub), k1 = min(k0 + per, nsub);
    for (uint32_t tt = blockIdx.x; tt < n_t; tt += gridDim.x) {
        uint32_t b, beg, end;
        group_tile(a, tt, b, beg, end);
        __syncthreads();                              // the previous tile's readers are done
        for (uint32_t k = t; k < nsub; k += kGPThreads) gcur[k] = a.tcount[(size_t)tt * nsub + k];
        for (uint32_t c0 = beg; c0 < end; c0 += kGChunk) {
            const uint32_t c1 = min(c0 + kGChunk, end);
            for (uint32_t k = t; k < kGPWaves * nsub; k += kGPThreads) hist[k] = 0;
            // this wave's 256 records of the chunk: 4 rounds, loaded together
            const uint32_t w0 = c0 + wid * 256u;
            Rec r[4];
            uint32_t sb[4], wr[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t j = w0 + (uint32_t)q * 64 + lane;
                r[q] = ld_rec<kNtRgRec>(in + (j < c1 ? j : c1 - 1));
            }
            __syncthreads();                          // hist zeroed (and gcur loaded)
            uint16_t* hw = hist + wid * nsub;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t j = w0 + (uint32_t)q * 64 + lane;
                const bool act = j < c1;
                sb[q] = act ? region_of_rec<Codec>(L, r[q], a.shard_bits) & smask : 0u;
                const uint64_t m = wave_match(sb[q], (int)a.sub_bits, act);
                const uint32_t lr = popc_below(m);
                wr[q] = (uint32_t)hw[sb[q]] + lr;    // rank among this wave's records of the region
                wave_fence();
                if (act && lr == 0) hw[sb[q]] = (uint16_t)(wr[q] + (uint32_t)__popcll(m));
                wave_fence();
            }
            __syncthreads();
            // region-major, then wave: each region's start in the chunk, each wave's offset in it
            uint32_t sum = 0;
            for (uint32_t k = k0; k < k1; ++k) {
                uint32_t run = 0;
                for (uint32_t w = 0; w < (uint32_t)kGPWaves; ++w) {
                    const uint32_t v = hist[w * nsub + k];
                    hist[w * nsub + k] = (uint16_t)run;
                    run += v;
                }
                tsub[k] = run;                        // (the region's count, for now)
                sum += run;
            }
            uint32_t base = block_exclusive_scan<kGPThreads>(sum, s_tmp, nullptr);
            for (uint32_t k = k0; k < k1; ++k) {
                const uint32_t c = tsub[k];
                tsub[k] = base;
                base += c;
            }
            __syncthreads();
            // sorted slots in LDS; the final position of every pass-0 position
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t j = w0 + (uint32_t)q * 64 + lane;
                if (j < c1) {
                    const uint32_t o = (uint32_t)hist[wid * nsub + sb[q]] + wr[q];
                    stg[tsub[sb[q]] + o] = r[q];
                    ssub[tsub[sb[q]] + o] = (uint16_t)sb[q];
                    st<kNtScPos>(a.pos_out + j, gcur[sb[q]] + o);
                }
            }
            __syncthreads();
            // the chunk in sorted order: runs of consecutive records per region
            for (uint32_t i = t; i < c1 - c0; i += kGPThreads) {
                const uint32_t k = ssub[i];
                st_rec<false>(out + gcur[k] + (i - tsub[k]), stg[i]);
            }
            __syncthreads();
            // the tile's cursors past this chunk
            for (uint32_t k = k0; k < k1; ++k) {
                const uint32_t nx = k + 1 < nsub ? tsub[k + 1] : c1 - c0;
                gcur[k] += nx - tsub[k];
            }
        }
    }
}

hipError_t launch_group(const GroupArgs& a, bool wide, hipStream_t s) {
    if (a.n_bins0 == 0 || a.sub_bits > (uint32_t)kMaxDigitBits || a.max_tiles == 0)
        return hipErrorInvalidValue;
    const size_t nsub = (size_t)1 << a.sub_bits;
    const size_t lds = kGroupWaves * nsub * sizeof(uint32_t);
    // one wave per tile: a persistent grid over the (device-counted) tiles
    const dim3 gw(persistent_grid((a.max_tiles + kGroupWaves - 1) / kGroupWaves, 8)), b(kGroupThreads);
    hipLaunchKernelGGL(k_gtiles, dim3(1), dim3(1024), 0, s, a);
    if (wide) hipLaunchKernelGGL(k_gcount<CodecW>, gw, b, lds, s, a);
    else hipLaunchKernelGGL(k_gcount<CodecC>, gw, b, lds, s, a);
    hipLaunchKernelGGL(k_gscan, dim3(a.n_bins0), b, nsub * sizeof(uint32_t), s, a);
    if (a.sub_bits <= kGLdsMaxSub && !(RL_ABLATION(a) & kAblGroupSeq)) {
        const dim3 gp(persistent_grid((a.max_tiles + 1) / 2, 4)), bp(kGPThreads);
        if (wide) hipLaunchKernelGGL(k_gplace_lds<CodecW>, gp, bp, gplace_lds_bytes<RecW>(a.sub_bits), s, a);
        else hipLaunchKernelGGL(k_gplace_lds<CodecC>, gp, bp, gplace_lds_bytes<RecC>(a.sub_bits), s, a);
        return hipGetLastError();
    }
    if (wide) hipLaunchKernelGGL(k_gplace<CodecW>, gw, b, lds, s, a);
    else hipLaunchKernelGGL(k_gplace<CodecC>, gw, b, lds, s, a);
    return hipGetLastError();
}

}  // namespace rl
