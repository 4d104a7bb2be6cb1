// rl_partition.hip — stable partition of a batch's requests into bin order (upsweep, scans,
// the two scatters, segment bases, routed ranges), for gfx950. Every pass reads the caller's
// request arrays; a two-pass batch's bins are then grouped by region in rl_group.hip.
#include "rl_kcommon.hpp"

#pragma clang fp contract(off)

namespace rl {

// Dynamic LDS of the kernels below; the kernels carve their pointers, and the launchers size
// the launch, with the same functions.
// k_upsweep: hist[bins] u32, then the route table when routing.
__host__ __device__ inline size_t upsweep_lds_bytes(uint32_t bins, bool route) {
    return bins * sizeof(uint32_t) + (route ? sizeof(RouteLds) : 0);
}
// k_scatter: cntw[bins] u64 (a bin's per-wave counts of the round, one byte each), cur[bins] u32
// (its next slot).
__host__ __device__ inline size_t scatter_lds_bytes(uint32_t bins) {
    return bins * (sizeof(uint64_t) + sizeof(uint32_t));
}
// k_scatter_split: the same, then from the next 16-B boundary stg[2][kTileThreads] records and
// sdg[2][kTileThreads] u16 digits (the two stages).
__host__ __device__ inline size_t scatter_stage_off(uint32_t bins) {
    return (scatter_lds_bytes(bins) + 15) & ~(size_t)15;
}
template <class Codec>
__host__ __device__ inline size_t scatter_split_lds_bytes(uint32_t bins) {
    return scatter_stage_off(bins) + 2 * kTileThreads * (sizeof(typename Codec::Rec) + sizeof(uint16_t));
}

// ------------------------------------------------------------------ 1. upsweep
// DIG: the pass stores each element's digit for the scatter (routing).
template <bool DIG>
__global__ __launch_bounds__(kTileThreads) void k_upsweep(PartArgs a) {
    // dynamic LDS (upsweep_lds_bytes): the histogram of this pass's bins, then the route table
    // when routing; sized to the pass so that 4 workgroups fit a CU at 8192 bins
    extern __shared__ uint32_t dyn_lds[];
    __shared__ LimLds L;
    const uint32_t t = threadIdx.x;
    const uint32_t bins = pass_bins(a);
    uint32_t* hist = dyn_lds;
    RouteLds& R = *(RouteLds*)((char*)dyn_lds + upsweep_lds_bytes(bins, false));
    load_lim_lds(L, a.lims, a.n_lim);
    if (a.route_list) route_load(R, a.route_list);
    if (blockIdx.x == 0 && t == 0) {
        BatchCtl* c = a.ctl;
        c->base_ms = floor_div_ms(a.now_ns[0]) - (1LL << 31);
        c->min_now_key = ~0ULL;
        c->max_now_key = 0;
        c->span_overflow = 0;
        c->n_esc = 0;
        c->allowed = c->distinct = c->invalid = c->cap_err = c->regions = c->cache_hits = 0;
        c->grow[0] = c->grow[1] = c->grow[2] = c->grow[3] = 0;
        c->table_bytes = 0;
        c->n_normal = a.n;                           // k_route_ranges lowers it when routing
        c->n_hot = 0;                                // k_hot_prep sets it when the hot path runs
        c->internal_err = 0;
        c->n_walk = 0;                               // k_hot_scan sets it when the hot path runs
    }
    const uint32_t n = a.n;
    for (uint32_t it = 0;; ++it) {
        const uint32_t tile = tile_at(it, a.n_tiles);
        if (tile >= a.n_tiles) break;
        for (uint32_t b = t; b < bins; b += kTileThreads) hist[b] = 0;
        __syncthreads();
        const uint32_t items = a.tile_items, T = items * (uint32_t)kTileThreads;
        if (tile * (uint64_t)T < n) {
#pragma unroll 8
            for (uint32_t r = 0; r < items; ++r) {
                const uint32_t i = tile * T + r * (uint32_t)kTileThreads + t;
                if (i < n) {
                    const uint32_t g = bin_of(a, i, L);
                    const uint32_t d = pass_digit(a, g, R);
                    atomicAdd(&hist[d], 1u);
                    if constexpr (DIG) a.digit[i] = (uint16_t)d;      // the scatter reads it back
                }
            }
        }
        __syncthreads();
        for (uint32_t b = t; b < bins; b += kTileThreads)
            a.counts[(size_t)b * a.n_tiles + tile] = hist[b];
    }
}

// ------------------------------------------------------------------ 2. scans
// Exclusive scan of each row of a [rows][cols] matrix (one block per row).
__global__ __launch_bounds__(256) void k_scan_rows(const uint32_t* in, uint32_t* out,
                                                   uint32_t cols, uint32_t* totals) {
    __shared__ uint32_t tmp[4];
    const size_t row = blockIdx.x;
    const uint32_t* src = in + row * cols;
    uint32_t* dst = out + row * cols;
    const uint32_t chunk = (cols + 255) / 256;
    const uint32_t beg = min(threadIdx.x * chunk, cols);
    const uint32_t end = min(beg + chunk, cols);
    uint32_t sum = 0;
    for (uint32_t k = beg; k < end; ++k) sum += src[k];
    uint32_t tot;
    uint32_t run = block_exclusive_scan<256>(sum, tmp, &tot);
    for (uint32_t k = beg; k < end; ++k) {
        const uint32_t v = src[k];
        dst[k] = run;
        run += v;
    }
    if (threadIdx.x == 0) totals[row] = tot;
}

// Single-block exclusive scan of a short array (<= a few million entries).
__global__ __launch_bounds__(1024) void k_scan_small(const uint32_t* in, uint32_t* out,
                                                     uint32_t len) {
    __shared__ uint32_t tmp[16];
    const uint32_t chunk = (len + 1023) / 1024;
    const uint32_t beg = min(threadIdx.x * chunk, len);
    const uint32_t end = min(beg + chunk, len);
    uint32_t sum = 0;
    for (uint32_t k = beg; k < end; ++k) sum += in[k];
    uint32_t run = block_exclusive_scan<1024>(sum, tmp, nullptr);
    for (uint32_t k = beg; k < end; ++k) {
        const uint32_t v = in[k];
        out[k] = run;
        run += v;
    }
}

// ------------------------------------------------------------------ 3. scatter
// Stable: a tile's elements are ranked in (round, wave, lane) order, which is the
// arrival order; tiles are ordered by the exclusive [bin][tile] scan. The inputs of
// round r+1 are loaded into registers before round r is ranked, so the global-load
// latency hides behind the two LDS barriers of a round.
//
// One request's inputs. They are passed by const& into inlined code and never copied: a
// register move would wait on its load.
struct ScatterIn {
    uint64_t key; int64_t now_ns; int32_t permits; uint32_t lim; uint32_t op; uint32_t dig;
    // Every load is unconditional (an absent array reads the key's bytes instead and the
    // value is dropped): a load under a branch leaves the wait-count pass unsure how many
    // loads are in flight, and it then waits for all of them — the whole prefetch ring and
    // every store before it — at the first use of any input.
    __device__ inline void load(const PartArgs& a, uint32_t i) {
        key = ld<kNtScIn>(a.key + i);
        now_ns = ld<kNtScIn>(a.now_ns + i);
        permits = ld<kNtScIn>(a.permits + i);
        const uint16_t* lp = a.limiter ? a.limiter + i : (const uint16_t*)(a.key + i);
        const uint8_t* op_p = a.op ? a.op + i : (const uint8_t*)(a.key + i);
        const uint16_t* dp = a.digit ? a.digit + i : (const uint16_t*)(a.key + i);
        lim = *lp;            // raw: masked where used (a select here would wait for it)
        op = *op_p;
        dig = ld<kNtScIn>(dp);
    }
    __device__ inline uint32_t lim_v(const PartArgs& a) const { return a.limiter ? lim : 0u; }
    __device__ inline uint32_t op_v(const PartArgs& a) const { return a.op ? op : 0u; }
    __device__ inline uint32_t dig_v(const PartArgs& a) const { return a.digit ? dig : 0u; }
};

// Earliest / latest now_ms of a workgroup's valid requests and whether one of them leaves the
// compact record's span, published to BatchCtl once per workgroup.
struct TimeRange {
    uint64_t mn = ~0ULL, mx = 0;
    bool overflow = false;
    template <class Codec>
    __device__ __forceinline__ void add(int64_t now_ms, int64_t base) {
        // only the compact record keeps now relative to base
        if constexpr (std::is_same<Codec, CodecC>::value) {
            const int64_t rel = now_ms - base;
            overflow |= rel < 0 || rel > 0xFFFFFFFFLL;
        }
        const uint64_t k = ord_key(now_ms);
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
    }
    // (every thread of the workgroup's WAVES waves) -> one atomic each
    template <int WAVES>
    __device__ __forceinline__ void publish(BatchCtl* ctl, uint64_t (&s_mm)[2][WAVES]) {
        const uint32_t t = threadIdx.x, lane = t & 63, wid = t >> 6;
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t a1 = __shfl_xor(mn, o, 64), b1 = __shfl_xor(mx, o, 64);
            mn = a1 < mn ? a1 : mn;
            mx = b1 > mx ? b1 : mx;
        }
        __syncthreads();
        if (lane == 0) { s_mm[0][wid] = mn; s_mm[1][wid] = mx; }
        const bool any_over = __syncthreads_or(overflow);
        if (t == 0) {
            for (int w = 1; w < WAVES; ++w) {
                mn = s_mm[0][w] < mn ? s_mm[0][w] : mn;
                mx = s_mm[1][w] > mx ? s_mm[1][w] : mx;
            }
            if (mn != ~0ULL) atomicMin((unsigned long long*)&ctl->min_now_key, (unsigned long long)mn);
            if (mx != 0) atomicMax((unsigned long long*)&ctl->max_now_key, (unsigned long long)mx);
            if (any_over) atomicOr(&ctl->span_overflow, 1u);
        }
    }
};

// Request i's record and its digit of this pass (a zero record, digit 0, past the batch).
template <class Codec>
__device__ __forceinline__ void encode_request(const PartArgs& a, const LimLds& L, int64_t base,
                                               const ScatterIn& in, uint32_t i, uint32_t n,
                                               TimeRange& tr, typename Codec::Rec& rec, uint32_t& d) {
    rec = typename Codec::Rec{};
    d = 0;
    if (i >= n) return;
    uint32_t lim = in.lim_v(a), op = in.op_v(a);
    const int32_t p = in.permits;
    const int64_t now_ms = floor_div_ms(in.now_ns);
    const bool lim_ok = lim < a.n_lim;
    if (!lim_ok) lim = 0;
    const bool invalid = !lim_ok || op > 2u || (op == 0u && p <= 0);
    if (op > 2u) op = 0;
    const uint64_t h = mix64(in.key);
    rec = Codec::enc(h, now_ms, base, p, op, lim, invalid);
    // an invalid request's now is never read: it neither widens the batch's time range nor
    // rejects the batch for its span
    if (!invalid) tr.add<Codec>(now_ms, base);
    // routing: the upsweep's digit (route-table lookup done once per request)
    d = a.digit ? in.dig_v(a)
                : (region_of(L, h, lim, a.shard_bits) >> a.digit_shift) & ((1u << a.digit_bits) - 1);
}

// One round's ranks: the position of this lane's element of bin d (active lanes), from the
// bin's next slot cur[d], the earlier waves' counts of the round (cntw[d]: the waves' bytes
// packed in one word, so a lane sums them with one read and two v_sad_u8) and the lane's rank
// among its own wave's elements of the bin (ballot match). Called by all waves `wid` of a
// ranking group together (two barriers); cur[d] moves past the round. no_match / no_barrier:
// the measurement-only variants (ranks then wrong), constants in the product kernels.
__device__ __forceinline__ uint32_t rank_round(uint64_t* cntw, uint32_t* cur, uint32_t d, int digit_bits,
                                               bool active, uint32_t lane, uint32_t wid,
                                               bool no_match, bool no_barrier) {
    const uint64_t m = no_match ? (1ULL << lane) : wave_match(d, digit_bits, active);
    const uint32_t lr = popc_below(m);
    const uint32_t cnt = (uint32_t)__popcll(m);
    const bool leader = active && lr == 0;
    if (leader) ((uint8_t*)&cntw[d])[wid] = (uint8_t)cnt;
    if (!no_barrier) __syncthreads();
    uint32_t pos = 0;
    if (active) {
        const uint64_t below = wid == 0 ? 0ULL : cntw[d] & ((1ULL << (8 * wid)) - 1);
        pos = cur[d] + lr + __builtin_amdgcn_sad_u8((uint32_t)below, 0u, 0u) +
              __builtin_amdgcn_sad_u8((uint32_t)(below >> 32), 0u, 0u);
    }
    if (!no_barrier) __syncthreads();
    if (leader) {
        atomicAdd(&cur[d], cnt);
        ((uint8_t*)&cntw[d])[wid] = 0;
    }
    return pos;
}

// The record output arrays: routed regions' records go straight to the final array, at a
// uniform element offset from the normal one. Selecting between the two kernel-argument
// pointers per lane let the compiler fold their reads into one vector load from the argument
// segment at a lane-chosen offset, followed by a vmcnt(0) wait in every round (a drain of the
// prefetched loads and of every store in flight); a pointer rebuilt from integers is a flat
// one, whose stores the wait-count pass cannot track either. An offset keeps both out.
template <class Rec>
__device__ inline void scatter_outputs(const PartArgs& a, Rec*& out_norm, int64_t& route_off,
                                       uint32_t& lo_route) {
    out_norm = (Rec*)a.rec_out;
    route_off = a.route_list ? (Rec*)a.rec_out_route - out_norm : 0;
    lo_route = a.route_list ? a.lo_bins : 0xFFFFFFFFu;
}

constexpr int kScatterDepth = 8;   // rounds of inputs in flight (divides tile_items)

template <class Codec>
__global__ __launch_bounds__(kTileThreads) void k_scatter(PartArgs a) {
    using Rec = typename Codec::Rec;
    static_assert(kTileThreads / 64 <= 8, "per-wave counts are packed 8 to a bin");
    extern __shared__ uint64_t dyn_lds64[];           // (scatter_lds_bytes)
    __shared__ LimLds L;
    __shared__ uint64_t s_mm[2][kTileThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const uint32_t bins = pass_bins(a);
    uint64_t* cntw = dyn_lds64;
    uint32_t* cur = (uint32_t*)(cntw + bins);
    load_lim_lds(L, a.lims, a.n_lim);
    const int64_t base = a.ctl->base_ms;
    // lanes past the batch store to the padding past it (a.n)
    const uint32_t n = a.n;
    const uint32_t last = n - 1;
    Rec* out_norm;
    int64_t route_off;
    uint32_t lo_route;
    scatter_outputs(a, out_norm, route_off, lo_route);
    TimeRange tr;
    for (uint32_t it = 0;; ++it) {
        const uint32_t tile = tile_at(it, a.n_tiles);
        if (tile >= a.n_tiles) break;
        const uint32_t tile0 = tile * a.tile_items * (uint32_t)kTileThreads;
        if (tile0 >= n) continue;                        // (workgroup-uniform)
        __syncthreads();     // previous tile's LDS users are done
        for (uint32_t b = t; b < bins; b += kTileThreads) {
            cur[b] = cursor_base(a, b, tile) + a.counts[(size_t)b * a.n_tiles + tile];
            cntw[b] = 0;
        }
        // kScatterDepth rounds of inputs in flight; out-of-range lanes re-load element n-1
        // so every wave issues the same loads and stores each round (static vmcnt counting)
        ScatterIn in[kScatterDepth];
#pragma unroll
        for (int k = 0; k < kScatterDepth; ++k) in[k].load(a, min(tile0 + (uint32_t)k * kTileThreads + t, last));
        __syncthreads();
        auto round = [&](const ScatterIn& in, int r) {
            const uint32_t i = tile0 + (uint32_t)r * kTileThreads + t;
            const bool active = i < n;
            Rec rec;
            uint32_t d;
            encode_request<Codec>(a, L, base, in, i, n, tr, rec, d);
            const uint32_t abl = RL_ABLATION(a);
            uint32_t pos = rank_round(cntw, cur, d, a.digit_bits, active, lane, wid,
                                      abl & kAblNoMatch, abl & kAblNoBarrier);
            if (abl & (kAblNoMatch | kAblNoBarrier)) pos = min(pos, n - 1);
            // inactive lanes write to the padding slot past n (buffers carry spare entries)
            uint32_t wpos = active ? pos : a.n + t;
            if (abl & kAblSeqRecStore) wpos = active ? i : a.n + t;
            // a routed region's records go straight to the final record array
            Rec* dst = out_norm + ((active && d >= lo_route ? route_off : 0) + wpos);
            if (!(abl & kAblNoRecStore)) st_rec<kNtScRec>(dst, rec);
            if (!(abl & kAblNoPosStore)) st<kNtScPos>(a.pos_out + (active ? i : a.n + t), pos);
        };
        // Unrolled by the prefetch depth so the input registers rotate without moves (a
        // move would wait on its load). vmcnt retires loads and stores in issue order, so
        // waiting for round r's inputs also waits for the scattered stores issued before
        // them: a deep ring spreads that store-ack latency over kScatterDepth rounds.
        for (int r = 0; r < (int)a.tile_items; r += kScatterDepth) {
#pragma unroll
            for (int k = 0; k < kScatterDepth; ++k) {
                round(in[k], r + k);
                in[k].load(a, min(tile0 + (uint32_t)(r + k + kScatterDepth) * kTileThreads + t, last));
            }
        }
    }
    tr.publish(a.ctl, s_mm);
}

// ------------------------------------------------------------------ 3b. split scatter
// The same stable partition with the global loads and the stores in different waves. gfx950
// has one vmcnt for vector loads and stores, retired in issue order: in k_scatter a wave's
// wait for its prefetched inputs also waits for the acks of every scattered record store it
// issued before them (no-store ablation on sw_zipf: scatter0 4.8 -> 2.8 ms). Here loader waves
// (threads kTileThreads..2*kTileThreads-1) keep kSplitDepth rounds of inputs in flight,
// encode each round and stage its records and digits in LDS one round ahead; the ranking
// waves (threads 0..kTileThreads-1) read them from LDS, rank, and store — they issue no
// global load inside a tile, so nothing ever waits behind their stores.
constexpr int kSplitDepth = 4;       // loader rounds in flight (divides tile_items)
// ABL (the measurement build's instantiations, its rl_tune ablate bits 20-25; results wrong): 1 no record
// store, 2 no position store, 4 records stored at their input index, 8 no ballot match,
// 16 no encode (the key as the record, digit 0 + lane), 32 whole sectors (each lane its
// record to both halves of its 32-B sector)
template <class Codec, int ABL = 0>
__global__ __launch_bounds__(2 * kTileThreads) void k_scatter_split(PartArgs a) {
    using Rec = typename Codec::Rec;
    constexpr int kRecV = (int)(sizeof(Rec) / 16);
    static_assert(sizeof(Rec) % 16 == 0, "records are whole 16-B vectors");
    extern __shared__ uint64_t dyn_lds64[];           // (scatter_split_lds_bytes)
    __shared__ LimLds L;
    __shared__ uint64_t s_mm[2][2 * kTileThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const bool loader = t >= (uint32_t)kTileThreads;          // (wave-uniform)
    const uint32_t lt = loader ? t - (uint32_t)kTileThreads : t;   // element within a round
    const uint32_t bins = pass_bins(a);
    uint64_t* cntw = dyn_lds64;                               // as k_scatter
    uint32_t* cur = (uint32_t*)(cntw + bins);
    Rec* stg = (Rec*)((char*)dyn_lds64 + scatter_stage_off(bins));   // [2][kTileThreads]
    uint16_t* sdg = (uint16_t*)(stg + 2 * kTileThreads);             // [2][kTileThreads]
    load_lim_lds(L, a.lims, a.n_lim);
    const int64_t base = a.ctl->base_ms;
    const uint32_t n = a.n;
    const uint32_t last = n - 1;
    Rec* out_norm;
    int64_t route_off;
    uint32_t lo_route;
    scatter_outputs(a, out_norm, route_off, lo_route);
    TimeRange tr;
    // (loaders) element i's record and digit
    auto encode = [&](const ScatterIn& in, uint32_t i, Rec& rec, uint32_t& d) __attribute__((always_inline)) {
        if constexpr (ABL & 16) {
            rec = Rec{};
            d = 0;
            if (i >= n) return;
            rec.h = in.key;
            d = (i & 63u) % (a.n_bins_pass ? a.n_bins_pass : 1u);
        } else {
            encode_request<Codec>(a, L, base, in, i, n, tr, rec, d);
        }
    };
    for (uint32_t it = 0;; ++it) {
        const uint32_t tile = tile_at(it, a.n_tiles);
        if (tile >= a.n_tiles) break;
        const uint32_t tile0 = tile * a.tile_items * (uint32_t)kTileThreads;
        if (tile0 >= n) continue;                        // (workgroup-uniform)
        __syncthreads();     // previous tile's LDS users are done
        // The two roles run separate loops with the same barriers (1 + 2 per round), so the
        // wait-count pass sees only the loaders' loads on one path and only the rankers'
        // stores on the other. Round r: rankers take round r from stage r & 1 while loaders
        // stage round r + 1 from the register ring (slot (r + 1) % depth) and reload that slot
        // with round r + 1 + depth (past the tile: the next tile's inputs, or element n - 1).
        if (loader) {
            ScatterIn in[kSplitDepth];
            for (uint32_t b = lt; b < bins; b += kTileThreads)
                cur[b] = cursor_base(a, b, tile) + a.counts[(size_t)b * a.n_tiles + tile];
#pragma unroll
            for (int k = 0; k < kSplitDepth; ++k) in[k].load(a, min(tile0 + (uint32_t)k * kTileThreads + lt, last));
            Rec r0;
            uint32_t d0;
            encode(in[0], tile0 + lt, r0, d0);           // round 0 staged before the loop
            stg[lt] = r0;
            sdg[lt] = (uint16_t)d0;
            in[0].load(a, min(tile0 + (uint32_t)kSplitDepth * kTileThreads + lt, last));
            __syncthreads();
            auto stage = [&](int r, ScatterIn& nxt) __attribute__((always_inline)) {
                // (the last round stages the next tile's first, unread: that tile's prologue
                // writes stage 0 again after its first barrier)
                const uint32_t i = tile0 + (uint32_t)(r + 1) * kTileThreads + lt;
                Rec nr;
                uint32_t nd;
                encode(nxt, i, nr, nd);
                const uint32_t sl = (uint32_t)((r + 1) & 1) * kTileThreads + lt;
                stg[sl] = nr;
                sdg[sl] = (uint16_t)nd;
                nxt.load(a, min(i + (uint32_t)kSplitDepth * kTileThreads, last));
                __syncthreads();
                __syncthreads();
            };
            for (int r = 0; r < (int)a.tile_items; r += kSplitDepth) {
#pragma unroll
                for (int k = 0; k < kSplitDepth; ++k) stage(r + k, in[(k + 1) % kSplitDepth]);
            }
        } else {
            for (uint32_t b = lt; b < bins; b += kTileThreads) cntw[b] = 0;
            __syncthreads();
            for (int r = 0; r < (int)a.tile_items; ++r) {
                const uint32_t i = tile0 + (uint32_t)r * kTileThreads + lt;
                const bool active = i < n;
                const uint32_t sl = (uint32_t)(r & 1) * kTileThreads + lt;
                u32x4_t rv[kRecV];                        // the record, kept in registers
#pragma unroll
                for (int k = 0; k < kRecV; ++k) rv[k] = ((const u32x4_t*)stg)[sl * kRecV + k];
                const uint32_t d = sdg[sl];
                const uint32_t pos = rank_round(cntw, cur, d, a.digit_bits, active, lane, wid,
                                                (ABL & 8) != 0, false);
                const uint32_t wpos = (ABL & 4) ? (active ? i : a.n + lt) : active ? min(pos, last) : a.n + lt;
                Rec* dst = out_norm + ((active && d >= lo_route && !(ABL & 4) ? route_off : 0) + wpos);
                if constexpr ((ABL & 32) && kRecV == 1) {
                    // whole 32-B sectors: the lane writes its record to both halves of its
                    // sector (twice the store lanes, no partial sector)
                    u32x4_t* sec = (u32x4_t*)(out_norm + ((active && d >= lo_route ? route_off : 0) + (wpos & ~1u)));
                    sec[0] = rv[0];
                    sec[1] = rv[0];
                } else if constexpr (!(ABL & 1)) {
#pragma unroll
                    for (int k = 0; k < kRecV; ++k) ((u32x4_t*)dst)[k] = rv[k];
                }
                if constexpr (!(ABL & 2)) st<kNtScPos>(a.pos_out + (active ? i : a.n + lt), pos);
            }
        }
    }
    tr.publish(a.ctl, s_mm);
}

// ------------------------------------------------------------------ segmented pass 0
// From the row-scanned counts (exclusive prefix per bin over the tiles): each (bin, segment)
// run's count, its start — normal bins segment-major over [0, n_normal), routed bins
// bin-major after them, exactly where the unsegmented layout put them — and the cursor
// base a tile of that segment adds to its row prefix (seg_adj = start - prefix at the
// segment's first tile; modular arithmetic).
__global__ __launch_bounds__(1024) void k_seg_base(const uint32_t* __restrict__ counts,
                                                   const uint32_t* __restrict__ bin_total,
                                                   const uint32_t* __restrict__ bin_base,
                                                   uint32_t bins, uint32_t lo, uint32_t nt,
                                                   uint32_t seg_tiles, uint32_t S, uint32_t* seg_adj,
                                                   uint32_t* seg_start, uint32_t* seg_cnt) {
    __shared__ uint32_t tmp[16];
    auto pre = [&](uint32_t b, uint32_t s) -> uint32_t {
        const uint32_t t0 = s * seg_tiles;
        return t0 < nt ? counts[(size_t)b * nt + t0] : bin_total[b];
    };
    const uint32_t N = S * lo;
    const uint32_t per = (N + 1023) / 1024;
    const uint32_t i0 = min(threadIdx.x * per, N), i1 = min(i0 + per, N);
    uint32_t sum = 0;
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t s = i / lo, b = i % lo;
        sum += pre(b, s + 1) - pre(b, s);
    }
    uint32_t run = block_exclusive_scan<1024>(sum, tmp, nullptr);
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t s = i / lo, b = i % lo;
        const uint32_t p0 = pre(b, s), c = pre(b, s + 1) - p0;
        seg_start[b * S + s] = run;
        seg_cnt[b * S + s] = c;
        seg_adj[b * S + s] = run - p0;
        run += c;
    }
    for (uint32_t b = lo + threadIdx.x; b < bins; b += 1024)
        for (uint32_t s = 0; s < S; ++s) {
            const uint32_t p0 = pre(b, s);
            seg_adj[b * S + s] = bin_base[b];
            seg_start[b * S + s] = bin_base[b] + p0;
            seg_cnt[b * S + s] = pre(b, s + 1) - p0;
        }
}

// ------------------------------------------------------------------ routing helpers
// After the pass-0 scan: the routed bins' ranges and the number of normal records, which the
// grouping, the region stage and the unpermute read on device.
__global__ __launch_bounds__(1024) void k_route_ranges(const uint32_t* __restrict__ route_list,
                                                       const uint32_t* __restrict__ bin_base,
                                                       const uint32_t* __restrict__ bin_total,
                                                       uint32_t lo_bins, uint32_t* route_start,
                                                       uint32_t* route_cnt, BatchCtl* ctl) {
    for (uint32_t i = threadIdx.x; i < kRouteSlots; i += blockDim.x) {
        const bool used = route_list[i] != kNone;
        const uint32_t bn = lo_bins + (used ? route_list[kRouteSlots + i] : 0u);
        route_start[i] = used ? bin_base[bn] : 0u;
        route_cnt[i] = used ? bin_total[bn] : 0u;
    }
    if (threadIdx.x == 0) ctl->n_normal = bin_base[lo_bins];
}

// ------------------------------------------------------------------ launchers
hipError_t launch_upsweep(const PartArgs& a, hipStream_t s) {
    dim3 grid(persistent_grid(a.n_tiles, a.up_per_cu ? a.up_per_cu : 4)), block(kTileThreads);
    const uint32_t bins = pass_bins(a);
    if (bins > (1u << kMaxDigitBits)) return hipErrorInvalidValue;
    const size_t lds = upsweep_lds_bytes(bins, a.route_list != nullptr);
    if (a.digit) hipLaunchKernelGGL(k_upsweep<true>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(k_upsweep<false>, grid, block, lds, s, a);
    return hipGetLastError();
}

#if RL_MEASURE   // the k_scatter_split<CodecC, ABL != 0> kernels exist in the measurement build only
template <int ABL>
static void scatter_split_abl(const PartArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((k_scatter_split<CodecC, ABL>), grid, dim3(2 * kTileThreads), lds, s, a);
}
#endif

hipError_t launch_scatter(const PartArgs& a, bool wide, hipStream_t s) {
    dim3 grid(persistent_grid(a.n_tiles, a.sc_per_cu ? a.sc_per_cu : 1)), block(kTileThreads);
    const uint32_t bins = pass_bins(a);
    if (bins > (1u << kMaxDigitBits)) return hipErrorInvalidValue;
    const dim3 b2(2 * kTileThreads);
    const size_t lc = scatter_split_lds_bytes<CodecC>(bins), lw = scatter_split_lds_bytes<CodecW>(bins);
#if RL_MEASURE
    if (a.sc_split && (RL_ABLATION(a) >> 20) && !wide) {
        switch ((RL_ABLATION(a) >> 20) & 63u) {
            case 1: scatter_split_abl<1>(a, grid, lc, s); break;
            case 2: scatter_split_abl<2>(a, grid, lc, s); break;
            case 3: scatter_split_abl<3>(a, grid, lc, s); break;
            case 4: scatter_split_abl<4>(a, grid, lc, s); break;
            case 8: scatter_split_abl<8>(a, grid, lc, s); break;
            case 16: scatter_split_abl<16>(a, grid, lc, s); break;
            case 27: scatter_split_abl<27>(a, grid, lc, s); break;
            case 32: scatter_split_abl<32>(a, grid, lc, s); break;
            default: return hipErrorInvalidValue;
        }
    } else
#endif
    if (a.sc_split && !RL_ABLATION(a)) {
        if (wide) hipLaunchKernelGGL((k_scatter_split<CodecW>), grid, b2, lw, s, a);
        else hipLaunchKernelGGL((k_scatter_split<CodecC>), grid, b2, lc, s, a);
    } else {
        if (wide) hipLaunchKernelGGL((k_scatter<CodecW>), grid, block, scatter_lds_bytes(bins), s, a);
        else hipLaunchKernelGGL((k_scatter<CodecC>), grid, block, scatter_lds_bytes(bins), s, a);
    }
    return hipGetLastError();
}

hipError_t launch_scan_rows(const uint32_t* in, uint32_t* out, uint32_t rows, uint32_t cols,
                            uint32_t* totals, hipStream_t s) {
    hipLaunchKernelGGL(k_scan_rows, dim3(rows), dim3(256), 0, s, in, out, cols, totals);
    return hipGetLastError();
}

hipError_t launch_scan_small(const uint32_t* in, uint32_t* out, uint32_t len, hipStream_t s) {
    hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, s, in, out, len);
    return hipGetLastError();
}

hipError_t launch_seg_base(const uint32_t* counts, const uint32_t* bin_total,
                           const uint32_t* bin_base, uint32_t bins, uint32_t lo_bins,
                           uint32_t n_tiles, uint32_t seg_tiles, uint32_t n_segs,
                           uint32_t* seg_adj, uint32_t* seg_start, uint32_t* seg_cnt, hipStream_t s) {
    if (seg_tiles == 0 || (size_t)(n_segs - 1) * seg_tiles >= n_tiles || lo_bins > bins)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_seg_base, dim3(1), dim3(1024), 0, s, counts, bin_total, bin_base, bins,
                       lo_bins, n_tiles, seg_tiles, n_segs, seg_adj, seg_start, seg_cnt);
    return hipGetLastError();
}

hipError_t launch_route_ranges(const uint32_t* route_list, const uint32_t* bin_base,
                               const uint32_t* bin_total, uint32_t lo_bins, uint32_t* route_start,
                               uint32_t* route_cnt, BatchCtl* ctl, hipStream_t s) {
    hipLaunchKernelGGL(k_route_ranges, dim3(1), dim3(1024), 0, s, route_list, bin_base, bin_total,
                       lo_bins, route_start, route_cnt, ctl);
    return hipGetLastError();
}

}  // namespace rl
