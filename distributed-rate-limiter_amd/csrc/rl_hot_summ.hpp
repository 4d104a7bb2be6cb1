// rl_hot_summ.hpp — hot regions, phases 0 and A: k_hot_prep (bounds and dominant keys of each
// listed region) and k_hot_summ (the chunk and group summaries the chains decide by; their word
// format is rl_hot_words.hpp's). Included by rl_hot.hpp.
#pragma once
#include "rl_hot_thresh.hpp"
#include "rl_hot_words.hpp"

namespace rl {

// Lane order = arrival order; chunk g of the listed regions -> (region i, chunk c).
__device__ inline uint32_t hot_region_of(const uint32_t* s_base, uint32_t hc, uint32_t g) {
    uint32_t lo = 0, hi = hc;                        // last i with s_base[i] <= g
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (s_base[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// Phase 0 (one wave per listed region): bounds, chunks and the dominant key of a sample
// of the region's first 64 records (a hot region is dominated by its hot key), and a
// second key when the sample says it holds >= kHot2MinRecords of the region.
constexpr uint32_t kHot2MinSample = 4;
constexpr uint32_t kHot2MinRecords = 32768;
template <class Codec>
__global__ __launch_bounds__(64) void k_hot_prep(RegionArgs a) {
    const uint32_t hc = min(a.hot_count[0], kHotMax);
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i == 0 && lane == 0) a.ctl->n_hot = hc;
    if (i >= hc) return;
    const uint32_t e = a.hot_list[i];
    uint32_t bin, start, end;
    if (e & kHotRoutedBit) {                      // routed: its own pass-0 bin
        const uint32_t r = e & ~kHotRoutedBit;
        bin = a.route_list[r];
        start = a.route_start[r];
        end = start + a.route_cnt[r];
    } else {
        bin = e;
        start = a.rstart[bin];
        end = start + (a.rend ? a.rend[bin] - start : a.rcount[bin]);
    }
    const typename Codec::Rec* recs = (const typename Codec::Rec*)a.rec;
    const int64_t base = a.ctl->base_ms;
    const uint32_t n0 = min(end - start, 64u);
    const bool act = lane < n0;
    uint64_t h = 0;
    bool ok = false;
    if (act) {
        const Req q = Codec::dec(recs[start + lane], base);
        h = q.h;
        ok = !q.invalid;
    }
    uint32_t cnt = 0;
    for (uint32_t k = 0; k < n0; ++k) cnt += (__shfl(h, (int)k, 64) == h) ? 1u : 0u;
    uint32_t key = (act && ok) ? (cnt << 6) | (63u - lane) : 0u;
    for (int o = 32; o > 0; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o, 64));
    const uint64_t tag = __shfl(h, (int)(63u - (key & 63u)), 64);
    // a second heavy key (two hot Zipf keys in one region): its own chain, or wave 1 would
    // apply its ~10^5 records 64 at a time (sw_zipf: a 398K-record region set the stage)
    uint32_t key2 = (act && ok && h != tag) ? (cnt << 6) | (63u - lane) : 0u;
    for (int o = 32; o > 0; o >>= 1) key2 = max(key2, (uint32_t)__shfl_xor((int)key2, o, 64));
    const uint64_t tag2 = __shfl(h, (int)(63u - (key2 & 63u)), 64);
    const uint32_t c1 = key >> 6, c2 = key2 >> 6;
    const bool two = c1 >= 2u && c2 >= kHot2MinSample &&
                     (uint64_t)(end - start) * c2 >= (uint64_t)kHot2MinRecords * n0;
    if (lane == 0) {
        HotInfo f;
        f.tag = tag; f.bin = bin; f.start = start; f.end = end;
        f.n_chunks = (end - start + kHotChunk - 1) / kHotChunk;
        f.chunk_base = 0;
        f.ok = (c1 >= 2u ? 1u : 0u) | (two ? 2u : 0u);
        f.n_groups = (f.n_chunks + 63) / 64;
        f.group_base = 0;
        f.tag2 = two ? tag2 : 0;
        a.hot_info[i] = f;
    }
}

// Phase A (one wave per group of 64 chunks, all CUs): what a chain needs to decide its key's
// records of a chunk (64 records) or a group (4096) without reading them: the time range of
// its plain acquires, and how many of its records need the exact path (peek / reset); the
// words are laid out in rl_hot_words.hpp. The wave keeps four chunks' records in flight.
__device__ inline uint64_t wave_min64(uint64_t v) { return wave_min_dpp<uint64_t>(v); }
__device__ inline uint64_t wave_max64(uint64_t v) { return wave_max_dpp<uint64_t>(v); }
__device__ inline uint32_t wave_min32(uint32_t v) { return wave_min_dpp<uint32_t>(v); }
__device__ inline uint32_t wave_max32(uint32_t v) { return wave_max_dpp<uint32_t>(v); }

template <class Codec>
__global__ __launch_bounds__(256) void k_hot_summ(RegionArgs a) {
    using Rec = typename Codec::Rec;
    __shared__ uint32_t s_base[kHotMax + 1];
    const uint32_t hc = min(a.hot_count[0], kHotMax);
    const uint32_t total = a.hot_total[1];
    for (uint32_t i = threadIdx.x; i < hc; i += 256) s_base[i] = a.hot_info[i].group_base;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const Rec* recs = (const Rec*)a.rec;
    const int64_t base = a.ctl->base_ms;
    const int64_t lo = batch_lo(a.ctl), hi = batch_hi(a.ctl);
    const uint64_t lanes_below = (1ULL << lane) - 1;
    for (uint32_t gg = blockIdx.x * 4 + wid; gg < total; gg += gridDim.x * 4) {
        const uint32_t i = hot_region_of(s_base, hc, gg);
        const HotInfo f = a.hot_info[i];
        const DevLimiter& L = a.lims[a.region_lim[f.bin]];
        const bool tb = L.algo == kAlgoTB;
        const int64_t maxp = L.max_permits;
        const bool two = (f.ok & 2u) != 0;
        const uint32_t c0 = (gg - s_base[i]) * 64, c1 = min(c0 + 64, f.n_chunks);
        uint64_t gmn[2] = {~0ULL, ~0ULL}, gmx[2] = {0ULL, 0ULL};
        uint32_t gfl[2] = {0u, 0u};                      // seen in the group: 1 special, 2 hot, 4 early, 8 rest
        // allow-walk table of each key (slot 2 i + k): the first plain acquire of 1 and of at
        // most 2 permits in each ms, found once per (chunk, ms) and merged by atomicMin over
        // the chunks. The group's walk flags (hotw::kWalkUnordered, judged against the chunks
        // before in the group: wcarry; hotw::kWalkWide) keep the chain off the walk.
        const bool walk_on = walk_table_on(a, i, f, L, lo, hi);
        int64_t wcarry[2] = {INT64_MIN, INT64_MIN};
        uint32_t wflag[2] = {0u, 0u};
        auto load = [&](uint32_t c) { return recs[min(f.start + c * kHotChunk + lane, f.end - 1)]; };
        auto chunk = [&](const Rec& r, uint32_t c) {
            const uint32_t j = f.start + c * kHotChunk + lane;
            const bool valid = j < f.end;
            const Req q = Codec::dec(r, base);
            const bool acq = q.op == (uint32_t)kOpAcquire;
            const bool hot0 = valid && (f.ok & 1u) && !q.invalid && q.h == f.tag;
            const bool hot1 = two && valid && !q.invalid && q.h == f.tag2;
            uint64_t w[hotw::kEntryWords];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint32_t ow = hotw::key_words((uint32_t)k);
                if (k == 1 && !two) {                     // (wave-uniform) no second key: its words
                    const uint64_t no = hotw::chunk_n_rest(w[2]);   // hold only key 0's rest count
                    w[ow + 0] = (uint64_t)INT64_MAX; w[ow + 1] = (uint64_t)INT64_MIN;
                    w[ow + 2] = hotw::chunk_counts(0u, 0u, 0u, (uint32_t)no); w[ow + 3] = hotw::rest_only(no);
                    gfl[1] |= no ? 8u : 0u;
                    break;
                }
                const bool hot = k ? hot1 : hot0;
                const bool early = hot && acq && tb && (int64_t)q.permits > maxp;
                const bool plain = hot && acq && !early;
                const bool special = hot && !acq;         // the key's peek / reset
                // n_rest: not the dominant key / neither key (invalid records included)
                const bool rest = valid && !hot0 && (k == 0 || !hot1);
                uint64_t mn = ~0ULL, mx = 0ULL;
                if (k == 0 || two) {                      // (wave-uniform)
                    if constexpr (std::is_same<Codec, CodecC>::value) {
                        // compact records: now = base + now_rel, so the 32-bit offsets order
                        // the same way and the reductions move half the bits
                        const uint32_t m32 = wave_min32(plain ? r.now_rel : ~0u);
                        const uint32_t x32 = wave_max32(plain ? r.now_rel : 0u);
                        if (__ballot(plain)) {
                            mn = ord_key(base + (int64_t)m32);
                            mx = ord_key(base + (int64_t)x32);
                        }
                    } else {
                        mn = wave_min64(plain ? ord_key(q.now_ms) : ~0ULL);
                        mx = wave_max64(plain ? ord_key(q.now_ms) : 0ULL);
                    }
                }
                if (walk_on && (k == 0 || two)) {                // (wave-uniform)
                    const uint64_t pm = __ballot(plain);
                    if (pm) {
                        const uint64_t bp = pm & lanes_below;
                        const int64_t tp = shfl64(q.now_ms, bp ? 63 - __builtin_clzll(bp) : (int)lane);
                        const bool ooo = plain && (bp ? tp : wcarry[k]) > q.now_ms;
                        wflag[k] |= (__ballot(ooo) ? hotw::kWalkUnordered : 0u) |
                                    (__ballot(plain && q.permits > 2) ? hotw::kWalkWide : 0u);
                        uint2* wt = a.walk_tab + (size_t)(2 * i + k) * walk_stride(lo, hi);
                        const uint32_t ix = (uint32_t)(q.now_ms - lo), rel = j - f.start;
                        const uint64_t b1 = __ballot(plain && q.permits == 1) & lanes_below;
                        const uint64_t b2 = __ballot(plain && q.permits <= 2) & lanes_below;
                        const int64_t t1 = shfl64(q.now_ms, b1 ? 63 - __builtin_clzll(b1) : (int)lane);
                        const int64_t t2 = shfl64(q.now_ms, b2 ? 63 - __builtin_clzll(b2) : (int)lane);
                        if (plain && q.permits == 1 && (!b1 || t1 != q.now_ms))
                            atomicMin(&wt[ix].x, rel);
                        if (plain && q.permits <= 2 && (!b2 || t2 != q.now_ms))
                            atomicMin(&wt[ix].y, rel);
                        wcarry[k] = (int64_t)readlane64((uint64_t)q.now_ms, 63u - (uint32_t)__builtin_clzll(pm));
                    }
                }
                const uint32_t ns = (uint32_t)__popcll(__ballot(special));
                const uint32_t nh = (uint32_t)__popcll(__ballot(hot));
                const uint32_t ne = (uint32_t)__popcll(__ballot(early));
                const uint32_t no = (uint32_t)__popcll(__ballot(rest));
                w[ow + 0] = hotw::min_word(mn);
                w[ow + 1] = hotw::max_word(mx);
                w[ow + 2] = hotw::chunk_counts(ns, nh, ne, no);
                w[ow + 3] = hotw::rest_only(no);
                gmn[k] = mn < gmn[k] ? mn : gmn[k];
                gmx[k] = mx > gmx[k] ? mx : gmx[k];
                gfl[k] |= (ns ? 1u : 0u) | (nh ? 2u : 0u) | (ne ? 4u : 0u) | (no ? 8u : 0u);
            }
            uint64_t v = w[0];                            // lanes 0-7: one 64-B store
#pragma unroll
            for (int k = 1; k < (int)hotw::kEntryWords; ++k) v = lane == (uint32_t)k ? w[k] : v;
            if (lane < hotw::kEntryWords) a.hot_summ[(size_t)(f.chunk_base + c) * hotw::kEntryWords + lane] = v;
        };
        Rec q0 = load(c0), q1 = load(c0 + 1), q2 = load(c0 + 2), q3 = load(c0 + 3);
        for (uint32_t c = c0; c < c1; c += 4) {
            chunk(q0, c);     q0 = load(c + 4);
            if (c + 1 >= c1) break;
            chunk(q1, c + 1); q1 = load(c + 5);
            if (c + 2 >= c1) break;
            chunk(q2, c + 2); q2 = load(c + 6);
            if (c + 3 >= c1) break;
            chunk(q3, c + 3); q3 = load(c + 7);
        }
        uint64_t v = 0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t ow = hotw::key_words((uint32_t)k);
            const uint64_t gw0 = hotw::min_word(gmn[k]), gw1 = hotw::max_word(gmx[k]);
            const uint64_t gw2 = hotw::group_flags(gfl[k] & 1u, gfl[k] & 2u, gfl[k] & 4u, wflag[k]);
            const uint64_t gw3 = hotw::rest_only(gfl[k] >> 3 & 1u);   // rest: kept through the verdict
            v = lane == ow ? gw0 : lane == ow + 1 ? gw1 : lane == ow + 2 ? gw2 : lane == ow + 3 ? gw3 : v;
        }
        if (lane < hotw::kEntryWords) a.hot_summ2[(size_t)gg * hotw::kEntryWords + lane] = v;
    }
}

}  // namespace rl
