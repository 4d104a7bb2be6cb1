// rl_table.hpp — how a key is found in a limiter's state table, and what a slot found there
// means, for the kernels off the decision path: retry-after and quota (rl_retry.hpp), key migration
// (rl_migrate.hip), the census (rl_usage.hip), export / import / growth / sweep
// (rl_state.hip), snapshot / ordered put (rl_snapshot.hip) and the table shrink
// (rl_shrink.hip). The decision path has its own region load (rl_region.hpp, rl_hot.hpp).
//
// Everything here encodes the HBM slot invariant stated above slot_free (rl_device.hpp): a slot
// is free iff all its words are zero, and a key sits before the first free slot of its probe
// sequence (linear from its 4-aligned home, wrapping inside its region).
#pragma once
#include "rl_kcommon.hpp"

namespace rl {

// ------------------------------------------------------------------ the region of a key
// The slots of one region and their cache words (null where the limiter keeps no cache).
struct TableRegion { RL_GLOBAL Slot* tab; RL_GLOBAL uint64_t* xtab; };
__device__ inline TableRegion table_region_at(const DevLimiter& L, size_t slot0) {
    return TableRegion{as_global((Slot*)L.table + slot0),
                       L.cache_table ? as_global((uint64_t*)L.cache_table + slot0) : nullptr};
}
__device__ inline TableRegion table_region(const DevLimiter& L, uint64_t tag, int shard_bits) {
    return table_region_at(L, region_slot0(tag, shard_bits, L.region_bits));
}

// ------------------------------------------------------------------ the quad probe
// Four lanes look one key up: lane `sub` of the quad loads slot `sub` of a 4-slot bucket as two
// 16-B loads plus its cache word (a probe step of a key is one 128-B line), and the quad finds
// the matching or the first free slot from the wave's ballots. The probe walks on bucket by
// bucket, at most kProbeBuckets of them. The caller owns the loop (and may issue the loads of
// several keys' home buckets ahead of their resolve steps).
typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));
constexpr uint32_t kProbeBuckets = kRegionSlots / 4;

struct QuadSlot { u64x2_t lo, hi; uint64_t x; };      // {tag, a}, {b, c}, the cache word

// lane `sub`'s slot of bucket m of tag h's probe sequence (< kRegionSlots: inside the region)
__device__ inline uint32_t quad_pos(uint64_t h, uint32_t m, uint32_t sub) {
    return (slot_home(h) + 4 * m + sub) & (kRegionSlots - 1);
}
__device__ inline QuadSlot quad_load(const TableRegion& R, uint32_t pos) {
    RL_GLOBAL const u64x2_t* sp = (RL_GLOBAL const u64x2_t*)(R.tab + pos);
    return QuadSlot{sp[0], sp[1], R.xtab ? R.xtab[pos] : 0};
}

// One bucket of the probe, by every lane of the wave (ballots). A quad still probing (`op`)
// that sees tag h or a free slot is done: found (`mine` on the lane whose slot `s` is the
// key's) or absent; otherwise it walks on.
__device__ inline void quad_resolve(bool& op, const QuadSlot& s, uint64_t h, uint32_t lane, bool& mine) {
    const uint32_t sub = lane & 3, qbase = lane & ~3u;
    bool match = false, isfree = false;
    if (op) {
        isfree = (s.lo.x | s.lo.y | s.hi.x | s.hi.y | s.x) == 0;
        match = !isfree && s.lo.x == h;
    }
    const uint32_t qm = (uint32_t)(__ballot(match) >> qbase) & 0xFu;
    const uint32_t qf = (uint32_t)(__ballot(isfree) >> qbase) & 0xFu;
    if (op && (qm | qf)) {
        // a match after a free slot of the same bucket cannot be the key's (invariant)
        const bool found = qm != 0 && (qf == 0 || __builtin_ctz(qm) < __builtin_ctz(qf));
        mine = found && match && sub == (uint32_t)__builtin_ctz(qm);
        op = false;
    }
}

// ------------------------------------------------------------------ what a slot holds
// A used slot is worth keeping (import, growth) or moving (migration) iff it holds state or a
// cache word; the rest are tombstones.
__device__ inline bool slot_holds_state(int algo, const Slot& v, uint64_t x) {
    return x != 0 || state_present(algo, v.b, v.c);
}

// The Redis keys of a slot that are live at `now`, oldest first (TB: the hash "tb:<key>",
// start = last refill, deadline last refill + 2w; SW: the counters "rl:<key>:<W>", deadline last
// INCR + w). (The same rule as one predicate, with the cache word: slot_live, rl_device.hpp.)
struct LiveBuckets {
    uint32_t n;                                  // TB 0..1, SW 0..2
    int64_t start[2], count[2], deadline[2];     // [0, n)
};
__device__ inline LiveBuckets live_buckets(const DevLimiter& L, const Slot& v, int64_t now) {
    LiveBuckets r;
    if (L.algo == kAlgoTB) {
        r.n = ((v.c & 1u) && !(now > (int64_t)v.b + L.ttl_ms)) ? 1u : 0u;
        r.start[0] = r.start[1] = (int64_t)v.b; r.count[0] = r.count[1] = 0;
        r.deadline[0] = r.deadline[1] = (int64_t)v.b + L.ttl_ms;
        return r;
    }
    const SW2 q = sw_unpack(v.a, v.b, v.c);
    const int64_t w = L.window_ms;
    const int64_t d1 = q.b1_start + q.b1_off + w, d0 = q.b1_start + q.b0_off;
    const bool l0 = q.b0_cnt != 0 && !(now > d0);            // bucket b1_start - w
    const bool l1 = q.b1_cnt != 0 && !(now > d1);
    r.n = (l0 ? 1u : 0u) + (l1 ? 1u : 0u);
    r.start[0] = l0 ? q.b1_start - w : q.b1_start; r.start[1] = q.b1_start;
    r.count[0] = l0 ? q.b0_cnt : q.b1_cnt;         r.count[1] = q.b1_cnt;
    r.deadline[0] = l0 ? d0 : d1;                  r.deadline[1] = d1;
    return r;
}

// ------------------------------------------------------------------ whole-region rebuild
// Shared by state import, table growth and the TTL sweep: one wave reads a region's 256 slots,
// keeps those `keep` accepts, re-inserts each from its home into the LDS stage `dest` picks
// for it (linear probing, as a batch's region load does) and later writes every slot of a stage
// back, so the HBM slot invariant holds afterwards. Stages are cleared (stage_clear) first.
struct RegionStage {
    alignas(16) uint64_t tag[kRegionSlots];
    uint64_t sa[kRegionSlots], sb[kRegionSlots], sc[kRegionSlots], sx[kRegionSlots];
    uint32_t occ[kRegionSlots];
};

__device__ inline void stage_clear(RegionStage& S, uint32_t lane) {
    for (uint32_t k = lane; k < kRegionSlots; k += 64) S.occ[k] = 0;
}

// Returns this lane's count of used slots that `keep` refused.
template <class TabPtr, class XPtr, class Keep, class Dest>
__device__ inline uint32_t stage_region(TabPtr tab, XPtr xt, uint32_t lane, Keep keep, Dest dest) {
    constexpr uint32_t NS = kRegionSlots;
    Slot img[NS / 64];
    uint64_t xim[NS / 64];
    bool kp[NS / 64];
    uint32_t dropped = 0;
#pragma unroll
    for (uint32_t i = 0; i < NS / 64; ++i) {
        img[i] = tab[lane + 64 * i];
        xim[i] = xt ? xt[lane + 64 * i] : 0;
        kp[i] = !slot_free(img[i], xim[i]) && keep(img[i], xim[i]);
        dropped += (!slot_free(img[i], xim[i]) && !kp[i]) ? 1u : 0u;
    }
    wave_fence();
#pragma unroll
    for (uint32_t i = 0; i < NS / 64; ++i) {
        if (!kp[i]) continue;
        RegionStage& S = dest(img[i]);
        uint32_t p = slot_home(img[i].tag);
        while (atomicCAS(&S.occ[p], 0u, 1u) != 0u) p = (p + 1) & (NS - 1);
        S.tag[p] = img[i].tag; S.sa[p] = img[i].a; S.sb[p] = img[i].b; S.sc[p] = img[i].c;
        S.sx[p] = xim[i];
    }
    wave_fence();
    return dropped;
}

// One slot inserted by one lane as stage_region's loop does, but giving up after a whole turn
// of the region: for a stage fed from several source regions (the table shrink's merge,
// rl_shrink.hip), where "the kept slots fit" is the caller's plan and not a property of one
// region. False: no free LDS slot in kRegionSlots steps (nothing was written).
__device__ inline bool stage_insert_bounded(RegionStage& S, const Slot& v, uint64_t x) {
    constexpr uint32_t NS = kRegionSlots;
    uint32_t p = slot_home(v.tag);
    for (uint32_t step = 0; step < NS; ++step, p = (p + 1) & (NS - 1)) {
        if (atomicCAS(&S.occ[p], 0u, 1u) != 0u) continue;
        S.tag[p] = v.tag; S.sa[p] = v.a; S.sb[p] = v.b; S.sc[p] = v.c;
        S.sx[p] = x;
        return true;
    }
    return false;
}

// One image put into a staged region by the whole wave (state import, rl_put_keys and the
// ordered put of rl_snapshot.hip): it replaces the slot holding its tag, else claims the first
// free slot of its probe sequence. False: the region has neither (nothing changes).
__device__ inline bool stage_put(RegionStage& S, const Slot& im, uint64_t x, uint32_t lane) {
    constexpr uint32_t NS = kRegionSlots;
    const uint32_t home = slot_home(im.tag);
    int32_t p = -1;
    for (uint32_t b = 0; b < NS / 64 && p < 0; ++b) {    // probe order = (b, lane)
        const uint32_t s = (home + b * 64 + lane) & (NS - 1);
        const bool used = (S.occ[s] & kOccUsed) != 0;
        const uint64_t fre = __ballot(!used);
        const uint64_t hit = __ballot(used && S.tag[s] == im.tag);
        const uint64_t before = fre ? ((fre & (0 - fre)) - 1) | (fre & (0 - fre)) : ~0ULL;
        const uint64_t h = hit & before;                  // a hit before the first free slot
        if (h) p = (int32_t)((home + b * 64 + (uint32_t)__builtin_ctzll(h)) & (NS - 1));
        else if (fre) p = (int32_t)((home + b * 64 + (uint32_t)__builtin_ctzll(fre)) & (NS - 1));
    }
    if (p >= 0 && lane == 0) {
        S.occ[p] = kOccUsed;
        S.tag[p] = im.tag; S.sa[p] = im.a; S.sb[p] = im.b; S.sc[p] = im.c;
        S.sx[p] = x;
    }
    wave_fence();
    return p >= 0;
}

template <class TabPtr, class XPtr>
__device__ inline void write_region(const RegionStage& S, TabPtr tab, XPtr xt, uint32_t lane) {
    for (uint32_t k = lane; k < kRegionSlots; k += 64) {
        Slot v{0, 0, 0, 0};
        uint64_t x = 0;
        if (S.occ[k] & kOccUsed) {
            x = S.sx[k];
            v = slot_used(Slot{S.tag[k], S.sa[k], S.sb[k], S.sc[k]}, x);
        }
        tab[k] = v;
        if (xt) xt[k] = x;
    }
}

}  // namespace rl
