// rl_snapshot.hip — whole-table snapshot and ordered put (rl_snapshot_keys(_device),
// rl_put_keys_device; include/rl_engine.h). The rules both sides rest on (which regions a call
// writes, when a put's input is in ordered form) are in rl_snapshot.hpp.
//
// Snapshot: one wave per region. Lane l reads slots j * 64 + l, j = 0..3, each as two 16-B loads
// plus its cache word (quad_load); four ballots of slot_holds_state give the region's image count
// and every image's rank in slot order. Three launches on one stream, no host read in between:
//   k_snap_regions<false>  count[r] for every region of the call
//   k_snap_scan            offset[] = exclusive scan of count[] (one workgroup; a call has at most
//                          kSnapMaxRegions regions), and the header from the cut rule
//   k_snap_regions<true>   region r, if it fits (snap_fits), writes its images as three 16-B
//                          stores each at out[offset[r] + rank]
// The table is read twice (40 B per slot each time) and 48 B per image are written.
//
// Ordered put: k_put_check computes every image's destination d(i) = (limiter, region), flags
// d(i) < d(i-1) and unknown limiters, and appends the first image of every run of equal d to a
// list (one atomic per wave; the list's order does not matter). k_put_apply reads the flags and
// the run count from device memory: unless the input was rejected, one wave per run stages the
// run's region (stage_region, as k_import), puts the run's images in array order (stage_put) and
// writes the region back. Ordered form makes a region the business of exactly one run, so no two
// waves write the same region. k_put_header then writes the caller's header.
#include "rl_snapshot.hpp"
#include "rl_table.hpp"

namespace rl {

static_assert(kSnapRegionSlots == kRegionSlots, "a cap of one region always makes progress");
static_assert((uint64_t)kSnapMaxRegions * kRegionSlots < (1ull << 32), "32-bit image offsets");
static_assert(sizeof(KeyImage) == 48, "an image is three 16-B words");

constexpr int kSnapThreads = 256;                 // four regions per workgroup
constexpr int kSnapScanThreads = 1024;

size_t snap_scratch_bytes() { return (size_t)kSnapMaxRegions * 8 + 32 + sizeof(PutCtl); }
SnapScratch snap_scratch_at(void* base) {
    SnapScratch sc;
    sc.count = (uint32_t*)base;
    sc.offset = sc.count + kSnapMaxRegions;
    sc.hdr = (uint64_t*)(sc.offset + kSnapMaxRegions);
    sc.ctl = (PutCtl*)(sc.hdr + 4);
    return sc;
}

template <bool EMIT>
__global__ __launch_bounds__(kSnapThreads) void k_snap_regions(SnapArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * (kSnapThreads / 64) + (threadIdx.x >> 6);   // wave-uniform
    if (r >= a.m) return;
    uint32_t at = 0;
    if constexpr (EMIT) {
        const uint32_t c = a.count[r];
        at = a.offset[r];
        if (c == 0 || !snap_fits(at, c, a.cap)) return;
    }
    const TableRegion R = table_region_at(a.L, (size_t)(a.region_begin + r) * kRegionSlots);
    QuadSlot s[kRegionSlots / 64];
    uint64_t held[kRegionSlots / 64];
#pragma unroll
    for (uint32_t j = 0; j < kRegionSlots / 64; ++j) s[j] = quad_load(R, j * 64 + lane);
    uint32_t n = 0;
#pragma unroll
    for (uint32_t j = 0; j < kRegionSlots / 64; ++j) {
        held[j] = __ballot(slot_holds_state(a.L.algo, Slot{s[j].lo.x, s[j].lo.y, s[j].hi.x, s[j].hi.y}, s[j].x));
        n += (uint32_t)__builtin_popcountll(held[j]);
    }
    if constexpr (!EMIT) {
        if (lane == 0) a.count[r] = n;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kRegionSlots / 64; ++j) {
            const uint64_t idx = (uint64_t)at + popc_below(held[j]);
            if (((held[j] >> lane) & 1) && idx < a.cap) {
                RL_GLOBAL u64x2_t* op = (RL_GLOBAL u64x2_t*)as_global(a.out + idx);
                op[0] = u64x2_t{unmix64(s[j].lo.x), s[j].lo.y};
                op[1] = s[j].hi;
                op[2] = u64x2_t{s[j].x, (uint64_t)a.lim};      // limiter, reserved = 0
            }
            at += (uint32_t)__builtin_popcountll(held[j]);
        }
    }
}

__global__ __launch_bounds__(kSnapScanThreads) void k_snap_scan(SnapArgs a) {
    __shared__ uint32_t tmp[kSnapScanThreads / 64];
    __shared__ uint32_t s_fit, s_images;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { s_fit = 0; s_images = 0; }
    uint32_t carry = 0, fit = 0, images = 0;
    for (uint32_t base = 0; base < a.m; base += kSnapScanThreads) {   // (uniform trip count)
        const uint32_t i = base + tid;
        const uint32_t c = i < a.m ? a.count[i] : 0u;
        uint32_t total = 0;
        const uint32_t at = carry + block_exclusive_scan<kSnapScanThreads>(c, tmp, &total);
        if (i < a.m) {
            a.offset[i] = at;
            if (snap_fits(at, c, a.cap)) { fit += 1; images += c; }
        }
        carry += total;
    }
    __syncthreads();
    if (fit) { atomicAdd(&s_fit, fit); atomicAdd(&s_images, images); }
    __syncthreads();
    if (tid == 0) {
        uint64_t h[4];
        snap_header(a.m, s_fit, s_images, a.m ? a.count[0] : 0u, a.regions_total, h);
        a.hdr[0] = h[0]; a.hdr[1] = h[1]; a.hdr[2] = h[2]; a.hdr[3] = h[3];
    }
}

hipError_t launch_snapshot(const SnapArgs& a, hipStream_t s) {
    const uint32_t grid = (a.m + kSnapThreads / 64 - 1) / (kSnapThreads / 64);
    if (a.m) hipLaunchKernelGGL(k_snap_regions<false>, dim3(grid), dim3(kSnapThreads), 0, s, a);
    hipLaunchKernelGGL(k_snap_scan, dim3(1), dim3(kSnapScanThreads), 0, s, a);
    if (a.m && a.cap) hipLaunchKernelGGL(k_snap_regions<true>, dim3(grid), dim3(kSnapThreads), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ ordered put
constexpr int kPutCheckThreads = 256;
constexpr uint32_t kPutApplyGrid = 4096;          // single-wave workgroups, striding over the runs

// d(i); `bad`: the image names a limiter the engine does not have
__device__ inline uint64_t put_dest(const PutArgs& a, uint32_t i, bool& bad) {
    const uint32_t lim = a.in[i].limiter;
    if (lim >= a.n_lim) { bad = true; return snap_dest(lim, 0); }
    return snap_dest_of(lim, mix64(a.in[i].key_hash), a.shard_bits, a.lims[lim].region_bits);
}

__global__ __launch_bounds__(kPutCheckThreads) void k_put_check(PutArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t g = (uint64_t)blockIdx.x * kPutCheckThreads + threadIdx.x;
    const bool active = g < a.n;
    const uint32_t i = (uint32_t)g;
    bool bad = false, head = false;
    uint32_t flags = 0;
    if (active) {
        bool bad_prev = false;
        const uint64_t d = put_dest(a, i, bad);
        const uint64_t d_prev = i ? put_dest(a, i - 1, bad_prev) : 0;
        head = snap_run_head(i == 0, d_prev, d);
        flags = (snap_out_of_order(i == 0, d_prev, d) ? kPutRejectOrder : 0u) |
                (bad ? kPutRejectLimiter : 0u);
    }
    if (flags) atomicOr(&a.ctl->rejected, flags);
    const uint64_t hm = __ballot(head);
    if (hm == 0) return;                              // (wave-uniform)
    const int leader = __builtin_ctzll(hm);
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(&a.ctl->n_heads, (uint32_t)__builtin_popcountll(hm));
    base = (uint32_t)__shfl((int)base, leader, 64);
    if (head) a.heads[base + popc_below(hm)] = i;     // (at most n heads)
}

__global__ __launch_bounds__(64) void k_put_apply(PutArgs a) {
    __shared__ RegionStage S;
    const uint32_t lane = threadIdx.x;
    if (a.ctl->rejected) return;                      // the table stays untouched
    const uint32_t n_heads = a.ctl->n_heads;
    RL_GLOBAL const u64x2_t* in = (RL_GLOBAL const u64x2_t*)as_global(a.in);
    for (uint32_t h = blockIdx.x; h < n_heads; h += gridDim.x) {
        const uint32_t i0 = a.heads[h];
        const uint32_t lim0 = a.in[i0].limiter;
        const uint64_t tag0 = mix64(a.in[i0].key_hash);
        const DevLimiter& L = a.lims[lim0];
        const int algo = L.algo, rbits = L.region_bits;
        const uint64_t d0 = snap_dest_of(lim0, tag0, a.shard_bits, rbits);
        const TableRegion R = table_region(L, tag0, a.shard_bits);
        stage_clear(S, lane);
        stage_region(R.tab, R.xtab, lane,
                     [&](const Slot& v, uint64_t x) { return slot_holds_state(algo, v, x); },
                     [&](const Slot&) -> RegionStage& { return S; });
        uint32_t failed = 0;
        for (uint64_t j0 = i0;; j0 += 64) {           // the run, 64 images at a time
            const uint64_t j = j0 + lane;
            u64x2_t w0{0, 0}, w1{0, 0}, w2{0, 0};
            bool in_run = false;
            if (j < a.n) {
                w0 = in[3 * j]; w1 = in[3 * j + 1]; w2 = in[3 * j + 2];
                w0.x = mix64(w0.x);                   // key_hash -> tag
                in_run = snap_dest_of((uint32_t)(w2.y & 0xFFFFu), w0.x, a.shard_bits, rbits) == d0;
            }
            const uint64_t out = __ballot(!in_run);
            const uint32_t cnt = out ? (uint32_t)__builtin_ctzll(out) : 64u;
            for (uint32_t t = 0; t < cnt; ++t) {      // in array order: the later duplicate wins
                const Slot im{readlane64(w0.x, t), readlane64(w0.y, t), readlane64(w1.x, t),
                              readlane64(w1.y, t)};
                if (!stage_put(S, im, readlane64(w2.x, t), lane)) ++failed;
            }
            if (cnt < 64) break;
        }
        write_region(S, R.tab, R.xtab, lane);
        if (lane == 0 && failed) atomicAdd(&a.ctl->n_failed, failed);
        wave_fence();                                 // the next run clears the stage
    }
}

__global__ void k_put_header(PutArgs a) {
    const uint32_t rej = a.ctl->rejected, failed = rej ? 0u : a.ctl->n_failed;
    a.hdr[0] = rej ? 0 : (uint64_t)a.n - failed;
    a.hdr[1] = failed;
    a.hdr[2] = rej;
    a.hdr[3] = a.n;
}

hipError_t launch_put_ordered(const PutArgs& a, hipStream_t s) {
    hipError_t he = hipMemsetAsync(a.ctl, 0, sizeof(PutCtl), s);
    if (he != hipSuccess) return he;
    if (a.n) {
        const uint32_t blocks = (uint32_t)(((uint64_t)a.n + kPutCheckThreads - 1) / kPutCheckThreads);
        hipLaunchKernelGGL(k_put_check, dim3(blocks), dim3(kPutCheckThreads), 0, s, a);
        hipLaunchKernelGGL(k_put_apply, dim3(a.n < kPutApplyGrid ? a.n : kPutApplyGrid), dim3(64), 0, s, a);
    }
    hipLaunchKernelGGL(k_put_header, dim3(1), dim3(1), 0, s, a);
    return hipGetLastError();
}

}  // namespace rl
