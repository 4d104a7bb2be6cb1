// rl_hot_fill.hpp — hot regions, phase C: k_hot_fill writes the results of the chunks the
// chains decided, from the verdict words (rl_hot_words.hpp). Included by rl_hot.hpp.
#pragma once
#include "rl_hot_thresh.hpp"
#include "rl_hot_words.hpp"

#pragma clang fp contract(off)

namespace rl {

// A chunk a chain's allow walk decided (hotw::verdict_walked): the key's records under the
// state in sm[0..2], but the allowed ones (hotw::verdict_allows / verdict_offset) and, after
// each, the state that allow leaves (TB: Lua :56-64; SW: the INCR of :114-116). Every lane runs
// it (the allowed records' times and permits are read from their lanes); `mine`: this lane
// holds the key's record.
template <class Res, bool TOK>
__device__ inline void walk_fill_key(const RegionArgs& a, const DevLimiter& L, const uint64_t* sm,
                                     uint64_t v, const Req& q, bool mine, uint32_t lane, uint32_t j) {
    const bool tb = L.algo == kAlgoTB;
    uint64_t ya = sm[0], yb = sm[1], yc = sm[2];        // the state after the allows so far
    uint64_t sa = ya, sb = yb, sc = yc;                  // this lane's: after the last allow before it
    bool at = false;
    double nt = 0.0, nt_at = 0.0;
    const uint32_t na = hotw::verdict_allows(v);
#pragma unroll 1
    for (uint32_t k = 0; k < na; ++k) {
        const uint32_t o = hotw::verdict_offset(v, k);
        const int64_t t_o = (int64_t)readlane64((uint64_t)q.now_ms, o);
        const int32_t p_o = __builtin_amdgcn_readlane(q.permits, (int)o);
        if (tb) {
            nt = tb_refill(L, t_o, ya, yb, yc) - (double)p_o;
            ya = (uint64_t)__double_as_longlong(nt); yb = (uint64_t)t_o; yc = 1;
        } else {
            sw_commit_allows(L, sw_geo(t_o, L), ya, yb, yc, 1u, t_o);
        }
        if (lane == o) { at = true; nt_at = nt; }
        if (lane >= o) { sa = ya; sb = yb; sc = yc; }
    }
    if (!mine) return;
    bool alw = false;
    int64_t rem;
    double tk = __builtin_nan("");
    if (tb && (int64_t)q.permits > L.max_permits) {
        rem = kRemUnknown;                                  // :110-116
    } else {
        alw = at;
        if (tb) {
            tk = at ? nt_at : tb_refill(L, q.now_ms, sa, sb, sc);
            rem = d2l(tk);
        } else {
            const int64_t r = L.max_permits - sw_estimate(sw_unpack(sa, sb, sc), sw_geo(q.now_ms, L),
                                                          q.now_ms, L.window_ms);
            rem = r > 0 ? r : 0;
        }
    }
    put_res<Res>(a, j, alw, rem);
    if (TOK) a.tok[j] = tk;
}

// Phase C (one wave per group of 64 chunks, all CUs): results of the chunks the chains
// decided. The group's chunk verdicts come in with one load per lane; a chunk holding only
// the dominant key's records is written without reading them (unless TB balances are out).
// WALK: the chunks of allow walks' verdicts only, which the other instance skips — their
// exact per-record arithmetic would otherwise set the register budget of every fill wave
// (80 VGPRs instead of 38).
template <class Codec, class Res, bool TOK, bool WALK>
__global__ __launch_bounds__(256) void k_hot_fill(RegionArgs a) {
    __shared__ uint32_t s_base[kHotMax + 1];
    const uint32_t hc = min(a.hot_count[0], kHotMax);
    const uint32_t total = a.hot_total[1];
    for (uint32_t i = threadIdx.x; i < hc; i += 256) s_base[i] = a.hot_info[i].group_base;
    __syncthreads();
    if (a.ctl->span_overflow != 0) return;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const typename Codec::Rec* recs = (const typename Codec::Rec*)a.rec;
    const int64_t base = a.ctl->base_ms;
    Res* res = (Res*)a.res;
    constexpr uint32_t EW = hotw::kEntryWords, K1 = hotw::key_words(1), V = hotw::kVerdictWord;
    for (uint32_t gg = blockIdx.x * 4 + wid; gg < total; gg += gridDim.x * 4) {
        const uint32_t i = hot_region_of(s_base, hc, gg);
        const HotInfo f = a.hot_info[i];
        const uint32_t c0 = (gg - s_base[i]) * 64, c1 = min(c0 + 64, f.n_chunks);
        const uint64_t* s2 = a.hot_summ2 + (size_t)gg * EW;
        const uint64_t g0 = s2[V], g1 = s2[K1 + V];
        // lane l: chunk c0 + l's verdict words of both keys
        const uint64_t* s1l = a.hot_summ + (size_t)(f.chunk_base + min(c0 + lane, c1 - 1)) * EW;
        const uint64_t cv0 = s1l[V], cv1 = s1l[K1 + V];
        const uint64_t any = WALK ? __ballot(c0 + lane < c1 && hotw::verdict_walked((hotw::verdict_decided(g0) ? 0u : cv0) | (hotw::verdict_decided(g1) ? 0u : cv1)))
                                  : __ballot(c0 + lane < c1 && (hotw::verdict_decided(g0 | cv0) || hotw::verdict_decided(g1 | cv1)));
        if (!any) continue;
        const DevLimiter& L = a.lims[a.region_lim[f.bin]];
        // a record of a key under a plain threshold verdict: denied with remaining 0 under the
        // state in sm[0..2] (a TB acquire above max_permits: rejected early, :110-116)
        auto plain_fill = [&](const uint64_t* sm, const Req& q, uint32_t j) {
            const bool early = L.algo == kAlgoTB && (int64_t)q.permits > L.max_permits;
            res[j] = (Res)pack_result(false, early ? kRemUnknown : 0);
            if (TOK) a.tok[j] = (L.algo == kAlgoTB && !early) ? tb_refill(L, q.now_ms, sm[0], sm[1], sm[2])
                                                             : __builtin_nan("");
        };
        for (uint64_t m = any; m; m &= m - 1) {
            const uint32_t l = (uint32_t)__builtin_ctzll(m);
            const uint32_t c = c0 + l;
            const uint64_t c0w = readlane64(cv0, l), c1w = readlane64(cv1, l);
            // per key k: decided as part of its group (state in the group summary), or alone
            const uint64_t v0 = hotw::verdict_decided(g0) ? hotw::with_rest_of(hotw::group_decision(g0), c0w) : c0w;
            const uint64_t v1 = hotw::verdict_decided(g1) ? hotw::group_decision(g1) : c1w;
            const uint32_t j = f.start + c * kHotChunk + lane;
            if (hotw::verdict_walked(v0 | v1)) {         // an allow walk's verdict (chunk level)
                if constexpr (!WALK) continue;
                const bool valid = j < f.end;
                const Req q = Codec::dec(recs[valid ? j : f.start], base);
                const uint64_t* s1 = a.hot_summ + (size_t)(f.chunk_base + c) * EW;
                const bool ok = valid && !q.invalid;
                if (hotw::verdict_walked(v0)) walk_fill_key<Res, TOK>(a, L, s1, v0, q, ok && q.h == f.tag, lane, j);
                if (hotw::verdict_walked(v1)) walk_fill_key<Res, TOK>(a, L, s1 + K1, v1, q, ok && q.h == f.tag2, lane, j);
                // (a key with a plain verdict beside a walked one: as below)
                if ((hotw::verdict_plain(v0) && q.h == f.tag) || (hotw::verdict_plain(v1) && q.h == f.tag2)) {
                    if (ok) plain_fill(q.h == f.tag ? (hotw::verdict_decided(g0) ? s2 : s1) : (hotw::verdict_decided(g1) ? s2 : s1) + K1, q, j);
                }
                continue;
            }
            if constexpr (WALK) continue;
            if (j >= f.end) continue;
            // the decided keys' records here are acquires (n_special == 0); TB permits > max
            // (early rejects) are the only ones not (deny, 0); other records are the chains'
            if (!TOK && hotw::verdict_whole_chunk(v0)) {  // every record is the dominant key's
                res[j] = (Res)pack_result(false, 0);
                continue;
            }
            const Req q = Codec::dec(recs[j], base);
            if (q.invalid) continue;
            const uint64_t* s1 = a.hot_summ + (size_t)(f.chunk_base + c) * EW;
            const uint64_t* sm;
            if (hotw::verdict_decided(v0) && q.h == f.tag) sm = hotw::verdict_decided(g0) ? s2 : s1;
            else if (hotw::verdict_decided(v1) && q.h == f.tag2) sm = (hotw::verdict_decided(g1) ? s2 : s1) + K1;   // (ok bit 1)
            else continue;                               // another key
            plain_fill(sm, q, j);
        }
    }
}

}  // namespace rl
