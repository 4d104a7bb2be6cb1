// rl_hot_chain.hpp — hot regions, phase B: the chain of one region (hot_chain: load, pass 1 per
// key, pass 2, write back) and its kernel k_hot_chains. Included by rl_hot.hpp.
#pragma once
#include "rl_hot_walk.hpp"

#pragma clang fp contract(off)

namespace rl {

// Load and rebuild the region image in LDS (as k_regions), then find or insert the chained
// keys' slots: s_hslot[k] is key k's slot, -1 when it has no chain or the region is full.
template <class Codec>
RL_PART void chain_load_region(const RegionArgs& a, RegionLds<Codec, true>& S, const HotInfo& f,
                               const DevLimiter& L, RL_GLOBAL Slot* tab, uint32_t lane, int32_t* s_hslot) {
    constexpr uint32_t NS = kRegionSlots;
    Slot img[NS / 64];
#pragma unroll
    for (uint32_t k = 0; k < NS / 64; ++k) {
        S.occ[lane + 64 * k] = 0;
        S.pm[lane + 64 * k] = 0;
        img[k] = tab[lane + 64 * k];
    }
    wave_fence();
#pragma unroll
    for (uint32_t k = 0; k < NS / 64; ++k) {
        const Slot v = img[k];
        if (slot_live(L, v, keep_from(a))) {
            uint32_t p = slot_home(v.tag);
            while (atomicCAS(&S.occ[p], 0u, 1u) != 0u) p = (p + 1) & (NS - 1);
            S.tag[p] = v.tag; S.sa[p] = v.a; S.sb[p] = v.b; S.sc[p] = v.c;
        }
    }
    wave_fence();
    int32_t hsl[2] = {-1, -1};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!((f.ok >> k) & 1u)) continue;              // (wave-uniform)
        const uint64_t tg = k ? f.tag2 : f.tag;
        const uint32_t p0 = slot_home(tg);
        int32_t hslot = -1;
        for (uint32_t m = 0; m < NS; ++m) {             // linear probing, as the rebuild
            const uint32_t p = (p0 + m) & (NS - 1);
            const uint32_t o = S.occ[p];
            if (!(o & 1u) || S.tag[p] == tg) { hslot = (int32_t)p; break; }
        }
        if (hslot >= 0 && !(S.occ[hslot] & 1u) && lane == 0) {
            S.occ[hslot] = 1u; S.tag[hslot] = tg; S.sa[hslot] = 0; S.sb[hslot] = 0; S.sc[hslot] = 0;
        }
        wave_fence();
        hsl[k] = hslot;
    }
    if (lane == 0) { s_hslot[0] = hsl[0]; s_hslot[1] = hsl[1]; }
}

// One step down the summaries with [T0, T1): of the entries in `todo` (lane = entry: a chunk of
// a group, or a group of 64), those before the first one the range does not cover (or that
// holds a peek / reset) are decided: each lane's gets the key's state, constant there, and
// `verdict` in `words`. Returns that first entry (64: none left) and takes it, and the ones
// before it, out of todo.
template <class KC>
RL_PART uint32_t descend(const KC& k, uint64_t& todo, bool special, int64_t mn, int64_t mx,
                         uint64_t* words, uint64_t verdict) {
    const uint32_t lane = k.e.lane;
    const bool skip = !special && mn >= k.T0 && mx < k.T1;
    const uint64_t nsk = todo & ~__ballot(skip);
    const uint32_t fst = nsk ? (uint32_t)__builtin_ctzll(nsk) : 64u;
    if (((todo >> lane) & 1u) && lane < fst) {
        words[0] = k.sa; words[1] = k.sb; words[2] = k.sc;
        words[3] = verdict;
    }
    if (fst == 64u) return fst;
    todo &= fst == 63u ? 0ULL : ~((2ULL << fst) - 1);
    return fst;
}

// level 1: the chunks of one group of 64; the undecided ones are detailed
template <class KC>
RL_PART void descend_group(KC& k, uint32_t grp) {
    auto& e = k.e;
    const uint32_t c = grp * 64 + e.lane;
    const bool has = c < e.f.n_chunks;
    uint64_t* sm = e.summ_at(c) + k.ow;
    const ulonglong2 v01 = *(const ulonglong2*)sm;
    const uint64_t v2 = sm[2];
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    uint32_t ns = 0, ne = 0, nh = 0;
    if (has) {
        mn = (int64_t)v01.x;
        mx = (int64_t)v01.y;
        ns = hotw::chunk_n_special(v2);
        nh = hotw::chunk_n_hot(v2);
        ne = hotw::chunk_n_early(v2);
        e.any_hot |= nh != 0;
    }
    const uint64_t verdict = hotw::threshold_verdict(hotw::chunk_n_rest(v2), ne != 0);
    uint64_t todo = __ballot(has && nh != 0);
    while (todo) {
        const uint32_t fst = descend(k, todo, ns != 0, mn, mx, sm, verdict);
        if (fst == 64u) break;
        if (e.dbg.on) {
            const int64_t fmn = (int64_t)readlane64((uint64_t)mn, fst);
            const int64_t fmx = (int64_t)readlane64((uint64_t)mx, fst);
            e.dbg.n_fb += fmn < k.T0 ? 1u : 0u;
            e.dbg.n_late += fmx >= k.T1 ? 1u : 0u;
        }
        detail(k, grp * 64 + fst, mn, mx, ns, todo);
    }
}

// level 2: 64 groups per test, the next 64 in flight; the undecided ones are descended
template <class KC>
RL_PART void descend_region(KC& k) {
    auto& e = k.e;
    const uint32_t lane = e.lane;
    ulonglong2 nx01 = *(const ulonglong2*)(e.grp_at(lane) + k.ow);
    uint64_t nx2 = e.grp_at(lane)[k.ow + 2], nx3 = e.grp_at(lane)[k.ow + 3];
    for (uint32_t g0 = 0; g0 < e.f.n_groups; g0 += 64) {
        const uint32_t g = g0 + lane;
        const bool has = g < e.f.n_groups;
        uint64_t* sg = e.grp_at(g) + k.ow;
        const ulonglong2 v01 = nx01;
        const uint64_t v2 = nx2, v3 = nx3;
        nx01 = *(const ulonglong2*)(e.grp_at(g + 64) + k.ow);
        nx2 = e.grp_at(g + 64)[k.ow + 2];
        nx3 = e.grp_at(g + 64)[k.ow + 3];
        const int64_t mn = (int64_t)v01.x, mx = (int64_t)v01.y;
        const bool nh = hotw::group_has_hot(v2);
        e.any_hot |= has && nh;
        const uint64_t verdict = hotw::group_verdict(v3, hotw::group_has_early(v2));
        uint64_t todo = __ballot(has && nh);
        while (todo) {
            const uint32_t fst = descend(k, todo, hotw::group_has_special(v2), mn, mx, sg, verdict);
            if (fst == 64u) break;
            descend_group(k, g0 + fst);
        }
    }
}

// Pass 1 for key kk: the key's records decided, by the allow walk or down the summaries.
template <int A, class Env>
RL_PART void chain_pass1(Env& e, uint32_t kk) {
    KeyChain<A, Env> k(e, kk);
    const uint64_t c_p1 = e.dbg.now();
    k.retarget();
    k.pre = e.chunk_rec(0);
    if (!walk(k)) descend_region(k);
    e.dbg.add(e.dbg.cyc_pass1, c_p1);
}

// Pass 2: every other key of the region in arrival order, 64 records at a time through
// wave_apply.
template <int A, class Env>
RL_PART void chain_pass2(Env& e) {
    using Codec = typename Env::CodecT;
    using Rec = typename Env::Rec;
    const RegionArgs& a = e.a;
    const HotInfo& f = e.f;
    const uint32_t lane = e.lane;
    const uint32_t pad = a.n_total + lane;
    const uint32_t rest_w = hotw::rest_word(e.hot_ok2);
    const uint64_t c_p2 = e.dbg.now();
    uint32_t head = 0, count = 0;                     // LDS ring (wave-uniform)
    SparseSrc sp{nullptr, nullptr, 0, false};         // the whole image is in LDS
    auto apply64 = [&](uint32_t valid_n) {
        const bool v = lane < valid_n;
        const uint32_t ri = (head + (v ? lane : 0u)) % kRing;
        uint32_t n_hits = 0;                          // (no local cache on the hot path)
        const Applied ap = wave_apply<Codec, A, false>(a, e.S, e.L, lane, e.S.ring[ri], v, e.S.ring_pos[ri], e.base,
                                                pad, e.n_allowed, e.n_invalid, e.n_caperr, e.n_rounds, n_hits, sp);
        if (v && !(RL_ABLATION(a) & kAblNoChainStores)) {
            put_res<typename Env::Res>(a, ap.j, ap.alw, ap.rem);
            if (Env::TOK) a.tok[ap.j] = ap.tok;
        }
    };
    auto take = [&](const Rec& r, uint32_t j, bool valid) {   // append other keys' records
        const bool other = valid && !e.is_hot(Codec::dec(r, e.base), valid);
        const uint64_t bal = __ballot(other);
        if (other) {
            const uint32_t k = (head + count + popc_below(bal)) % kRing;
            e.S.ring[k] = r;
            e.S.ring_pos[k] = j;
        }
        count += (uint32_t)__popcll(bal);
        e.dbg.n_other += lane == 0 ? (uint32_t)__popcll(bal) : 0u;
        wave_fence();
        if (count >= 64) {
            apply64(64);
            head = (head + 64) % kRing;
            count -= 64;
        }
    };
    // The chunks holding other keys' records, in arrival order, across groups: a
    // wave-uniform cursor over (block of 64 groups, group, chunk). Four chunks' records
    // are in flight (unrolled, so the prefetch registers rotate without moves): a region
    // whose second key is itself hot runs thousands of chunks through here, and one
    // chunk in flight left each of them waiting on its load (sw_zipf: a 398K-record
    // region ended the region stage 3.5 ms after the normal regions).
    uint32_t cg0 = 0, cgrp = 0;
    uint64_t cgtodo = 0, ctodo = 0;
    bool cdone = f.n_groups == 0;
    auto group_mask = [&](uint32_t g0) {
        const uint32_t g = g0 + lane;
        return __ballot(g < f.n_groups && (!e.hot_ok || hotw::group_has_rest(e.grp_at(g)[rest_w])));
    };
    if (!cdone) cgtodo = group_mask(0);
    auto next_chunk = [&]() -> uint32_t {
        while (!cdone && ctodo == 0) {
            if (cgtodo == 0) {
                cg0 += 64;
                if (cg0 >= f.n_groups) { cdone = true; break; }
                cgtodo = group_mask(cg0);
                continue;
            }
            cgrp = cg0 + (uint32_t)__builtin_ctzll(cgtodo);
            cgtodo &= cgtodo - 1;
            const uint32_t c = cgrp * 64 + lane;
            uint32_t no = 0;
            if (c < f.n_chunks) no = e.hot_ok ? hotw::verdict_n_rest(e.summ_at(c)[rest_w]) : 64u;
            ctodo = __ballot(no != 0);
        }
        if (cdone) return kNone;
        const uint32_t cc = cgrp * 64 + (uint32_t)__builtin_ctzll(ctodo);
        ctodo &= ctodo - 1;
        return cc;
    };
    auto rec_of = [&](uint32_t cc) {
        return e.recs[cc == kNone ? f.start : min(f.start + cc * kHotChunk + lane, f.end - 1)];
    };
    auto take_chunk = [&](const Rec& r, uint32_t cc) {
        const uint32_t j = f.start + cc * kHotChunk + lane;
        take(r, j, j < f.end);
    };
    uint32_t k0 = next_chunk(), k1 = next_chunk(), k2 = next_chunk(), k3 = next_chunk();
    Rec r0 = rec_of(k0), r1 = rec_of(k1), r2 = rec_of(k2), r3 = rec_of(k3);
    while (k0 != kNone) {
        take_chunk(r0, k0); k0 = next_chunk(); r0 = rec_of(k0);
        if (k1 == kNone) break;
        take_chunk(r1, k1); k1 = next_chunk(); r1 = rec_of(k1);
        if (k2 == kNone) break;
        take_chunk(r2, k2); k2 = next_chunk(); r2 = rec_of(k2);
        if (k3 == kNone) break;
        take_chunk(r3, k3); k3 = next_chunk(); r3 = rec_of(k3);
    }
    if (count > 0) apply64(count);
    e.dbg.add(e.dbg.cyc_pass2, c_p2);
}

// the passes of one algorithm: wave 0 the chains of the keys that have one, then (SPLIT: wave 1
// beside them) every other key
template <int A, bool SPLIT, class Env>
RL_PART void chain_passes(Env& e, uint32_t wv) {
    if (wv == 0 && e.hot_ok) chain_pass1<A>(e, 0u);
    if (wv == 0 && e.hot_ok2) chain_pass1<A>(e, 1u);
    if (!SPLIT || wv == 1) chain_pass2<A>(e);
}

// Phase B (one single-wave workgroup per listed region, beside k_regions). Pass 1 goes down the
// region's summaries in arrival order with the hot key's threshold pair: a group of 64
// chunks, or a chunk, whose hot-key times all lie in [T0, T1) has its hot records decided
// without being read (verdict + the key's state go back into the summary for k_hot_fill);
// the other chunks are processed one by one (fast check, then the sequential run of the
// key's state changes). Pass 1 runs again for a second dominant key when the region
// holds one (HotInfo::ok bit 1). Pass 2 then applies every other key of the region in
// arrival order, 64 records at a time through wave_apply. (A workgroup of one wave per pass
// waited for its wave slots on one CU beside the normal regions: sw_zipf's later chains
// started ~4 ms into the stage.)
// SPLIT (two-wave workgroups): wave 0 loads the region and runs pass 1, wave 1 runs pass 2
// beside it on the same LDS image (pass 1 touches only its keys' slots, pass 2 never those)
// and exits, handing its debug words over in LDS; wave 0 waits for it and writes back.
template <class Codec, class Res, bool TOK, bool SPLIT>
RL_PART void hot_chain(const RegionArgs& a, uint32_t i, RegionLds<Codec, true>& S) {
    using Rec = typename Codec::Rec;
    constexpr uint32_t NS = kRegionSlots;
    __shared__ int32_t s_hslot[2];
    __shared__ uint64_t s_p2[3];                      // SPLIT: wave 1 done, its cycles, records
    const uint32_t hc = min(a.hot_count[0], kHotMax);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = SPLIT ? threadIdx.x >> 6 : 0u;
    if (i >= hc) return;
    // the passes are sequential critical paths beside thousands of normal-region waves
    __builtin_amdgcn_s_setprio(3);
    const HotInfo f = a.hot_info[i];
    const uint32_t region = f.bin;                    // a bin is one region
    const DevLimiter L = a.lims[a.region_lim[region]];
    Chain<Codec, Res, TOK> ch{a, S, f, L, i, lane, uni(a.ctl->base_ms), uni(batch_lo(a.ctl)),
                              uni(batch_hi(a.ctl)), (const Rec*)a.rec};
    // ---- the whole batch rejected (see k_regions)
    if (a.ctl->span_overflow != 0) {
        Res* res = (Res*)a.res;
        for (uint32_t j = f.start + threadIdx.x; j < f.end; j += blockDim.x) {
            res[j] = (Res)pack_result(false, kRemInvalid);
            if (TOK) a.tok[j] = __builtin_nan("");
        }
        return;
    }
    ch.dbg.on = a.dbg != nullptr;
    ch.dbg.t_start = a.dbg ? __builtin_amdgcn_s_memrealtime() : 0;
    // ---- load the region, find the chained keys' slots
    RL_GLOBAL Slot* tab = as_global((Slot*)L.table + (size_t)(region - L.region_base) * NS);
    if (wv == 0) {
        chain_load_region(a, S, f, L, tab, lane, s_hslot);
        if (SPLIT && lane == 0) s_p2[0] = 0;
    }
    if (SPLIT) __syncthreads();
    else wave_fence();
    ch.hsl0 = s_hslot[0];
    ch.hsl1 = ch.hsl0 >= 0 ? s_hslot[1] : -1;
    ch.hot_ok = ch.hsl0 >= 0;
    ch.hot_ok2 = ch.hsl1 >= 0;
    // ---- pass 1 per key, pass 2
    if (L.algo == kAlgoTB) chain_passes<kAlgoTB, SPLIT>(ch, wv);
    else chain_passes<kAlgoSW, SPLIT>(ch, wv);
    // ---- reduce the statistics
    for (int off = 32; off > 0; off >>= 1) {
        ch.n_allowed += __shfl_xor(ch.n_allowed, off, 64);
        ch.n_invalid += __shfl_xor(ch.n_invalid, off, 64);
        ch.n_caperr += __shfl_xor(ch.n_caperr, off, 64);
    }
    if (lane == 0) {
        unsigned long long* st = a.stats + (size_t)(blockIdx.x & (kStatSlots - 1)) * kStWords;
        if (ch.n_allowed) atomicAdd(st + kStAllowed, (unsigned long long)ch.n_allowed);
        if (ch.n_invalid) atomicAdd(st + kStInvalid, (unsigned long long)ch.n_invalid);
        if (ch.n_caperr) atomicAdd(st + kStCapErr, (unsigned long long)ch.n_caperr);
        if (ch.n_internal) atomicOr(&a.ctl->internal_err, 1u);
    }
    if (SPLIT) {
        if (wv == 1) {                                // hand over, then leave the SIMD
            if (lane == 0) {
                s_p2[1] = ch.dbg.cyc_pass2; s_p2[2] = ch.dbg.n_other;
                __atomic_store_n(&s_p2[0], 1ULL, __ATOMIC_RELEASE);
            }
            return;
        }
        while (__atomic_load_n(&s_p2[0], __ATOMIC_ACQUIRE) == 0) __builtin_amdgcn_s_sleep(2);
        ch.dbg.cyc_pass2 = s_p2[1];
        ch.dbg.n_other = (uint32_t)s_p2[2];
    }
    // ---- write the region back, statistics
    const bool hot_touched = __any(ch.any_hot);
    if (lane == 0 && ch.hot_ok && hot_touched) S.occ[ch.hsl0] |= 2u;
    if (lane == 0 && ch.hot_ok2 && hot_touched) S.occ[ch.hsl1] |= 2u;
    wave_fence();
    uint32_t touched = 0, used = 0;
    for (uint32_t sl = lane; sl < NS; sl += 64) {
        const uint32_t o = S.occ[sl];
        Slot v{0, 0, 0, 0};
        if (o & kOccUsed) v = slot_used(Slot{S.tag[sl], S.sa[sl], S.sb[sl], S.sc[sl]});
        tab[sl] = v;
        touched += (o >> 1) & 1u;
        used += o & kOccUsed;
    }
    for (int off = 32; off > 0; off >>= 1) {
        touched += __shfl_xor(touched, off, 64);
        used += __shfl_xor(used, off, 64);
        ch.dbg.n_bisect += __shfl_xor(ch.dbg.n_bisect, off, 64);
    }
    if (lane == 0) {
        note_fill(a, region, used, ch.n_caperr != 0);
        unsigned long long* st = a.stats + (size_t)(blockIdx.x & (kStatSlots - 1)) * kStWords;
        atomicAdd(st + kStDistinct, (unsigned long long)touched);
        atomicAdd(st + kStRegions, 1ULL);
        atomicAdd(st + kStTableBytes, (unsigned long long)(2u * NS * 32u));
        if (a.dbg) ch.dbg.store(a.dbg + (size_t)region * kDbgWords, f.end - f.start);
    }
}

// The hot chains alone (single-wave workgroups), launched on a side stream of the device's
// highest priority just before the normal regions' launch, so they start first. They are a
// few hundred lone waves beside ~10^6 normal-region waves: a larger register budget costs
// no occupancy that matters: one wave per SIMD gives the walk's registers room (512 VGPRs,
// no spills).
constexpr int kChainMinWaves = 1;
template <class Codec, class Res, bool TOK, bool SPLIT>
__global__ __launch_bounds__(SPLIT ? 128 : 64, kChainMinWaves) void k_hot_chains(RegionArgs a) {
    __shared__ RegionLds<Codec, true> S;
    const uint32_t hc = min(a.hot_count[0], kHotMax);
    if (SPLIT) {
        // one chain per workgroup: wave 1 leaves after its pass (the grid covers the list)
        if (blockIdx.x < hc) hot_chain<Codec, Res, TOK, true>(a, blockIdx.x, S);
        return;
    }
    for (uint32_t i = blockIdx.x; i < hc; i += gridDim.x) {       // (workgroup-uniform)
        wave_fence();                                             // the last chain's LDS users
        hot_chain<Codec, Res, TOK, false>(a, i, S);
    }
}

}  // namespace rl
