// rl_topk.hip — exact heavy hitters of a device array of key hashes (rl_top_keys,
// include/rl_engine.h): the keys that occur at least min_count times, the k most frequent of
// them in (count descending, key ascending unsigned) order, and how many there are.
//
// Five launches on one stream over a scratch of fixed size (TopkScratch):
//   k_topk_clear    zeroes the sketch, empties the candidate table, zeroes the control words.
//   k_topk_pass<0>  sketch: streams the keys once and adds every key's multiplicity to one
//                   u32 cell in each of two rows of 2^22, chosen by two mixes of the key. A
//                   cell only overestimates its keys' counts.
//   k_topk_pass<1>  filter and count: streams the keys again; a key whose smaller cell is below
//                   min_count cannot qualify and is dropped, every other key is inserted or
//                   incremented in an open-addressed {key, count} table of 2^19 slots that
//                   admits 2^18 live keys (one more sets the overflow flag).
//   k_topk_compact  drops the table's entries below min_count (the sketch's false positives)
//                   and appends the others to a dense list of 65536, a workgroup's at a time;
//                   their number is n_heavy (one more sets the overflow flag).
//   k_topk_select   one workgroup: when more than k qualify, a radix select over the counts
//                   (4 x 8 bits, most significant first) and then, among the ties at the cut,
//                   over the keys (8 x 8 bits) finds the last element kept; the at most 4096
//                   kept ones are sorted in LDS (bitonic) and written with the header.
// The host form runs the passes once per staged chunk; the device form once over the array.
// rl_top_denied runs the same five launches with the passes' selector instantiation
// (k_topk_pass<PASS, true>): only the keys of the requests denied under one limiter enter.
//
// Both passes aggregate equal keys inside the workgroup before they touch global memory: a
// tile of 2048 keys goes into an LDS hash table {key, count} with LDS atomics, and the table is
// flushed with one global no-return atomic per distinct (workgroup, key, row) — the top key
// of Zipf 1.1 traffic is 11% of a sample, and as single increments it would be one contended
// word. A key seen at least kKeepMin times stays in the LDS table across tiles and is flushed
// when the workgroup ends (or when too many have gathered), so a hot key costs about one
// global atomic per workgroup, not one per tile.
//
// Empty slots: both tables mark an empty slot with the key ~0, so one 64-bit compare-and-swap
// claims or matches a slot and no lane ever waits for another lane to finish a claim. The key
// ~0 itself never enters a table: it is counted in a word of its own (an LDS word per tile,
// ctl.special in global memory) and joins the candidates in k_topk_compact. Every 64-bit value
// is therefore a legal key. Counts are u32 (n <= 2^31); every comparison is unsigned.
#include "rl_kcommon.hpp"
#include "rl_report.hpp"

namespace rl {

namespace {

constexpr uint64_t kEmptyKey = ~0ULL;
constexpr int kPassThreads = 256;
constexpr int kTileKeys = 2048;                    // keys a workgroup aggregates at a time
constexpr int kPerThread = kTileKeys / kPassThreads;
constexpr int kLdsSlots = 4096;                    // LDS table: <= kKeepMax + 256 kept + 2048 new
constexpr uint32_t kKeepMin = 8;                   // occurrences from which a key stays in LDS
constexpr uint32_t kKeepMax = 1024;                // kept keys above which everything is flushed
constexpr int kPassGridMax = 768;                  // 3 workgroups (48 KB of LDS each) per CU
constexpr int kSelThreads = 1024;

__device__ inline uint64_t mix_b(uint64_t key) {   // the second row's mix, independent of mix64(key)
    return mix64((key ^ 0x9E3779B97F4A7C15ULL) * 0xD6E8FEB86659FD93ULL + 0x2545F4914F6CDD1DULL);
}

__device__ inline uint32_t ld_relaxed(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- clear
__global__ __launch_bounds__(256) void k_topk_clear(TopkScratch sc) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint4* sk = reinterpret_cast<uint4*>(sc.sketch);
    for (uint32_t i = t; i < 2 * kTopkSketchCells / 4; i += stride) sk[i] = make_uint4(0, 0, 0, 0);
    for (uint32_t i = t; i < kTopkTableSlots; i += stride) {
        sc.tab_key[i] = kEmptyKey;
        sc.tab_cnt[i] = 0;
    }
    if (t < sizeof(TopkCtl) / 4) reinterpret_cast<uint32_t*>(sc.ctl)[t] = 0;
}

// ---------------------------------------------------------------- the two streaming passes
// One distinct key of a workgroup with its multiplicity c, sketch pass: one add per row.
__device__ inline void flush_sketch(const TopkScratch& sc, uint64_t key, uint32_t c) {
    const uint32_t c0 = (uint32_t)mix64(key) & (kTopkSketchCells - 1);
    const uint32_t c1 = (uint32_t)mix_b(key) & (kTopkSketchCells - 1);
    atomicAdd(sc.sketch + c0, c);
    atomicAdd(sc.sketch + kTopkSketchCells + c1, c);
}

// The same in the filter pass: dropped when the sketch rules it out, else inserted / incremented
// in the candidate table. A new key beyond kTopkStoreMax sets the overflow flag; after that
// nothing more is inserted (the result is void), so the table never fills: at most
// kTopkStoreMax plus one racing claim per resident thread (768 x 256) are ever live.
__device__ inline void flush_table(const TopkScratch& sc, uint64_t key, uint32_t c, uint64_t min_count) {
    const uint64_t h = mix64(key);
    const uint32_t e0 = sc.sketch[(uint32_t)h & (kTopkSketchCells - 1)];
    const uint32_t e1 = sc.sketch[kTopkSketchCells + ((uint32_t)mix_b(key) & (kTopkSketchCells - 1))];
    if ((uint64_t)(e0 < e1 ? e0 : e1) < min_count) return;
    TopkCtl* ctl = sc.ctl;
    if (ld_relaxed(&ctl->overflow)) return;
    if (key == kEmptyKey) {
        if (atomicAdd(&ctl->special, c) == 0 && atomicAdd(&ctl->live, 1u) >= kTopkStoreMax)
            atomicExch(&ctl->overflow, 1u);
        return;
    }
    uint32_t slot = (uint32_t)(h >> 40) & (kTopkTableSlots - 1);
    for (uint32_t probe = 0; probe < kTopkTableSlots; ++probe) {
        unsigned long long* kp = reinterpret_cast<unsigned long long*>(sc.tab_key + slot);
        unsigned long long old = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == kEmptyKey) {
            old = atomicCAS(kp, (unsigned long long)kEmptyKey, (unsigned long long)key);
            if (old == kEmptyKey) {                                  // claimed: a new live key
                if (atomicAdd(&ctl->live, 1u) >= kTopkStoreMax) atomicExch(&ctl->overflow, 1u);
                old = key;
            }
        }
        if (old == key) {
            atomicAdd(sc.tab_cnt + slot, c);
            return;
        }
        slot = (slot + 1) & (kTopkTableSlots - 1);
    }
    atomicExch(&ctl->overflow, 1u);                                  // unreachable: see above
}

template <int PASS>
__device__ inline void flush_one(const TopkScratch& sc, uint64_t key, uint32_t c, uint64_t min_count) {
    if (PASS == 0) flush_sketch(sc, key, c);
    else flush_table(sc, key, c, min_count);
}

// SEL: only the keys of the requests the selector takes (rl_top_denied) enter the LDS table; a
// lane whose request is not selected contributes nothing. Pass 0 counts the selected ones into
// ctl.selected, one add per workgroup. Without SEL the selector is not looked at.
template <int PASS, bool SEL>
__global__ __launch_bounds__(kPassThreads) void k_topk_pass(TopkScratch sc, const uint64_t* __restrict__ key,
                                                            TopkSel sel, uint32_t n, uint64_t min_count) {
    __shared__ unsigned long long l_key[kLdsSlots];
    __shared__ uint32_t l_cnt[kLdsSlots];
    __shared__ uint32_t l_special;                 // occurrences of the key ~0
    __shared__ uint32_t l_kept[3];                 // keys kept by a flush: read in round r at [r % 3],
                                                   // summed at [(r + 1) % 3], zeroed at [(r + 2) % 3]
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kLdsSlots; i += kPassThreads) { l_key[i] = kEmptyKey; l_cnt[i] = 0; }
    __shared__ uint32_t l_selected;                // SEL, pass 0: selected requests of this workgroup
    if (tid == 0) { l_special = 0; l_kept[0] = 0; l_kept[1] = 0; l_kept[2] = 0; l_selected = 0; }
    __syncthreads();

    const uint32_t tiles = (n + kTileKeys - 1) / kTileKeys;          // n <= 2^31: no wrap
    uint32_t round = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, ++round) {
        const bool last = tile + gridDim.x >= tiles;
        const uint32_t base = tile * kTileKeys;                      // < 2^31 + 2048
        uint64_t k[kPerThread];
        bool on[kPerThread];
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
            const uint32_t i = base + (uint32_t)j * kPassThreads + tid;
            on[j] = i < n;
            k[j] = on[j] ? key[i] : 0;
            if constexpr (SEL) {
                if (on[j]) {
                    const uint32_t lim = sel.limiter ? sel.limiter[i] : 0u;
                    const uint32_t op = sel.op ? sel.op[i] : 0u;
                    on[j] = report_row(lim, sel.n_lim) == sel.sel &&
                            report_class(lim, sel.n_lim, op, sel.permits[i], sel.allowed[i],
                                         sel.remaining[i]) == kRcDenied;
                }
            }
        }
        if constexpr (SEL && PASS == 0) {
            uint32_t mine = 0;
#pragma unroll
            for (int j = 0; j < kPerThread; ++j) mine += on[j] ? 1u : 0u;
            if (mine) atomicAdd(&l_selected, mine);
        }
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
            if (!on[j]) continue;
            if (k[j] == kEmptyKey) { atomicAdd(&l_special, 1u); continue; }
            uint32_t slot = (uint32_t)(mix64(k[j]) >> 20) & (kLdsSlots - 1);
            bool done = false;
            for (int probe = 0; probe < kLdsSlots && !done; ++probe) {
                // a plain read first: a key that is already there (every kept one) needs no CAS
                unsigned long long old = *(volatile unsigned long long*)&l_key[slot];
                if (old == kEmptyKey)
                    old = atomicCAS(&l_key[slot], (unsigned long long)kEmptyKey, (unsigned long long)k[j]);
                if (old == kEmptyKey || old == k[j]) {
                    atomicAdd(&l_cnt[slot], 1u);
                    done = true;
                }
                slot = (slot + 1) & (kLdsSlots - 1);
            }
            if (!done) flush_one<PASS>(sc, k[j], 1u, min_count);     // unreachable: the table has room
        }
        __syncthreads();
        // flush: everything on the last tile or when too many keys are being kept, else all
        // but the keys seen kKeepMin times (at most 256 new ones per tile)
        const bool keep = !last && l_kept[round % 3] <= kKeepMax;
        uint32_t kept = 0;
        for (uint32_t i = tid; i < kLdsSlots; i += kPassThreads) {
            const uint64_t kk = l_key[i];
            if (kk == kEmptyKey) continue;
            const uint32_t c = l_cnt[i];
            if (keep && c >= kKeepMin) { ++kept; continue; }
            flush_one<PASS>(sc, kk, c, min_count);
            l_key[i] = kEmptyKey;
            l_cnt[i] = 0;
        }
        if (tid == 0) {
            if (l_special) flush_one<PASS>(sc, kEmptyKey, l_special, min_count);
            l_special = 0;
            l_kept[(round + 2) % 3] = 0;
        }
        if (kept) atomicAdd(&l_kept[(round + 1) % 3], kept);
        __syncthreads();
    }
    if constexpr (SEL && PASS == 0) {                                // (behind the last tile's barrier)
        if (tid == 0 && l_selected) atomicAdd(&sc.ctl->selected, l_selected);
    }
}

// ---------------------------------------------------------------- compact
// Every workgroup takes kCompactChunk slots of the table, gathers its qualifying entries in LDS
// and reserves their place in the list with one atomic (single appends to ctl.heavy would be
// one contended word). Workgroup 0 also takes the key ~0's count.
constexpr uint32_t kCompactChunk = 2048;
__global__ __launch_bounds__(256) void k_topk_compact(TopkScratch sc, uint64_t min_count) {
    __shared__ uint64_t s_k[kCompactChunk + 1];
    __shared__ uint32_t s_c[kCompactChunk + 1];
    __shared__ uint32_t s_n, s_base;
    TopkCtl* ctl = sc.ctl;
    if (ctl->overflow) return;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (uint32_t j = tid; j < kCompactChunk; j += 256) {
        const uint32_t i = blockIdx.x * kCompactChunk + j;           // grid = slots / chunk
        const uint64_t kk = sc.tab_key[i];
        const uint32_t c = sc.tab_cnt[i];
        if (kk == kEmptyKey || (uint64_t)c < min_count) continue;
        const uint32_t p = atomicAdd(&s_n, 1u);
        s_k[p] = kk;
        s_c[p] = c;
    }
    if (blockIdx.x == 0 && tid == 0) {
        const uint32_t c = ctl->special;
        if (c != 0 && (uint64_t)c >= min_count) {
            const uint32_t p = atomicAdd(&s_n, 1u);
            s_k[p] = kEmptyKey;
            s_c[p] = c;
        }
    }
    __syncthreads();
    if (tid == 0) s_base = s_n ? atomicAdd(&ctl->heavy, s_n) : 0u;
    __syncthreads();
    for (uint32_t p = tid; p < s_n; p += 256) {
        const uint32_t pos = s_base + p;
        if (pos < kTopkCandidates) { sc.list_key[pos] = s_k[p]; sc.list_cnt[pos] = s_c[p]; }
        else atomicExch(&ctl->overflow, 1u);                         // more qualify than may
    }
}

// ---------------------------------------------------------------- select
// a before b in the result order: count descending, key ascending (unsigned)
__device__ inline bool before(uint32_t ca, uint64_t ka, uint32_t cb, uint64_t kb) {
    return ca != cb ? ca > cb : ka < kb;
}

// One radix-select digit: with hist[256] filled (and a barrier behind it), the digit d at which
// the running total of the digits taken in `descending` (255 first) or ascending order first
// reaches `want`; `want` is reduced by the elements of the digits before d. Two levels, sixteen
// groups of sixteen digits, so that the serial walk is 32 steps. Called by every thread; every
// thread gets the same answer.
__device__ inline uint32_t pick_digit(const uint32_t* hist, uint32_t* grp, bool descending, uint32_t& want) {
    if (threadIdx.x < 16) {
        uint32_t sum = 0;
        for (int i = 0; i < 16; ++i) sum += hist[threadIdx.x * 16 + i];
        grp[threadIdx.x] = sum;
    }
    __syncthreads();
    uint32_t acc = 0, g = descending ? 0u : 15u;                     // (the last group: want <= total)
    for (int s = 0; s < 16; ++s) {
        const uint32_t gg = descending ? 15u - (uint32_t)s : (uint32_t)s;
        if (acc + grp[gg] >= want) { g = gg; break; }
        acc += grp[gg];
    }
    for (int s = 0; s < 16; ++s) {
        const uint32_t d = g * 16 + (descending ? 15u - (uint32_t)s : (uint32_t)s);
        const uint32_t h = hist[d];
        if (acc + h >= want) { want -= acc; return d; }
        acc += h;
    }
    return g * 16 + (descending ? 0u : 15u);                         // unreachable
}

__global__ __launch_bounds__(kSelThreads) void k_topk_select(TopkScratch sc, uint32_t k, uint64_t n_in,
                                                             uint64_t* __restrict__ top_key,
                                                             uint64_t* __restrict__ top_count,
                                                             uint64_t* __restrict__ hdr,
                                                             uint32_t count_selected) {
    __shared__ uint64_t s_key[kTopkMax];
    __shared__ uint32_t s_cnt[kTopkMax];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_grp[16];
    __shared__ uint32_t s_fill;
    const uint32_t tid = threadIdx.x;
    const TopkCtl* ctl = sc.ctl;
    const uint64_t n = count_selected ? (uint64_t)ctl->selected : n_in;   // hdr[3]
    if (ctl->overflow) {
        if (tid == 0) { hdr[0] = 0; hdr[1] = 0; hdr[2] = 1; hdr[3] = n; }
        return;
    }
    const uint32_t m = ctl->heavy < kTopkCandidates ? ctl->heavy : kTopkCandidates;   // n_heavy
    const uint32_t n_out = m < k ? m : k;
    // the last element kept is (cut_c, cut_k): everything before it in the order, and itself
    uint32_t cut_c = 0;
    uint64_t cut_k = kEmptyKey;
    if (m > k) {
        uint32_t want = k;                                           // rank of the cut, 1-based, in what remains
        uint32_t pc = 0;                                             // count: the digits fixed so far
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            const uint32_t himask = shift == 24 ? 0u : ~0u << (shift + 8);
            for (uint32_t i = tid; i < m; i += kSelThreads) {
                const uint32_t c = sc.list_cnt[i];
                if ((c & himask) == pc) atomicAdd(&s_hist[(c >> shift) & 255u], 1u);
            }
            __syncthreads();
            pc |= pick_digit(s_hist, s_grp, true, want) << shift;
            __syncthreads();
        }
        cut_c = pc;
        uint64_t pk = 0;                                             // key: among count == cut_c, ascending
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            const uint64_t himask = shift == 56 ? 0ULL : ~0ULL << (shift + 8);
            for (uint32_t i = tid; i < m; i += kSelThreads) {
                if (sc.list_cnt[i] != cut_c) continue;
                const uint64_t kk = sc.list_key[i];
                if ((kk & himask) == pk) atomicAdd(&s_hist[(uint32_t)(kk >> shift) & 255u], 1u);
            }
            __syncthreads();
            pk |= (uint64_t)pick_digit(s_hist, s_grp, false, want) << shift;
            __syncthreads();
        }
        cut_k = pk;
    }
    // gather the kept ones, pad to a power of two with (count 0, key ~0): last in the order
    uint32_t p2 = 1;
    while (p2 < n_out) p2 <<= 1;
    if (tid == 0) s_fill = 0;
    for (uint32_t i = tid; i < p2; i += kSelThreads) { s_key[i] = kEmptyKey; s_cnt[i] = 0; }
    __syncthreads();
    for (uint32_t i = tid; i < m; i += kSelThreads) {
        const uint32_t c = sc.list_cnt[i];
        const uint64_t kk = sc.list_key[i];
        if (m > k && before(cut_c, cut_k, c, kk)) continue;          // after the cut
        const uint32_t pos = atomicAdd(&s_fill, 1u);
        if (pos < kTopkMax) { s_key[pos] = kk; s_cnt[pos] = c; }     // always: exactly n_out pass
    }
    __syncthreads();
    for (uint32_t len = 2; len <= p2; len <<= 1) {
        for (uint32_t inc = len >> 1; inc > 0; inc >>= 1) {
            for (uint32_t t = tid; t < p2 / 2; t += kSelThreads) {
                const uint32_t lo = (t / inc) * (inc << 1) + (t % inc), hi = lo + inc;
                const bool up = (lo & len) == 0;                     // this run ends in result order
                const uint32_t ca = s_cnt[lo], cb = s_cnt[hi];
                const uint64_t ka = s_key[lo], kb = s_key[hi];
                if (before(cb, kb, ca, ka) == up) {
                    s_cnt[lo] = cb; s_key[lo] = kb;
                    s_cnt[hi] = ca; s_key[hi] = ka;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < n_out; i += kSelThreads) {
        top_key[i] = s_key[i];
        top_count[i] = (uint64_t)s_cnt[i];
    }
    if (tid == 0) { hdr[0] = n_out; hdr[1] = m; hdr[2] = 0; hdr[3] = n; }
}

}  // namespace

size_t topk_scratch_bytes() {
    return sizeof(TopkCtl) + 2 * (size_t)kTopkSketchCells * 4 + (size_t)kTopkTableSlots * 12 +
           (size_t)kTopkCandidates * 12 + (size_t)kTopkMax * 16 + 4 * 8;
}

TopkScratch topk_scratch_at(void* base) {
    // 8-byte members first; every offset is a multiple of 16
    TopkScratch sc{};
    char* p = (char*)base;
    sc.ctl = (TopkCtl*)p;             p += sizeof(TopkCtl);
    sc.tab_key = (uint64_t*)p;        p += (size_t)kTopkTableSlots * 8;
    sc.list_key = (uint64_t*)p;       p += (size_t)kTopkCandidates * 8;
    sc.out_key = (uint64_t*)p;        p += (size_t)kTopkMax * 8;
    sc.out_cnt = (uint64_t*)p;        p += (size_t)kTopkMax * 8;
    sc.out_hdr = (uint64_t*)p;        p += 4 * 8;
    sc.sketch = (uint32_t*)p;         p += 2 * (size_t)kTopkSketchCells * 4;
    sc.tab_cnt = (uint32_t*)p;        p += (size_t)kTopkTableSlots * 4;
    sc.list_cnt = (uint32_t*)p;
    return sc;
}

hipError_t launch_topk_clear(const TopkScratch& sc, hipStream_t s) {
    hipLaunchKernelGGL(k_topk_clear, dim3(1024), dim3(256), 0, s, sc);
    return hipGetLastError();
}

hipError_t launch_topk_pass(const TopkScratch& sc, int pass, const uint64_t* key, uint32_t n,
                            uint64_t min_count, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t tiles = (n + kTileKeys - 1) / kTileKeys;
    const uint32_t grid = tiles < (uint32_t)kPassGridMax ? tiles : (uint32_t)kPassGridMax;
    const TopkSel none{};
    if (pass == 0) hipLaunchKernelGGL((k_topk_pass<0, false>), dim3(grid), dim3(kPassThreads), 0, s, sc, key, none, n, min_count);
    else hipLaunchKernelGGL((k_topk_pass<1, false>), dim3(grid), dim3(kPassThreads), 0, s, sc, key, none, n, min_count);
    return hipGetLastError();
}

hipError_t launch_topk_pass_sel(const TopkScratch& sc, int pass, const uint64_t* key, const TopkSel& sel,
                                uint32_t n, uint64_t min_count, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t tiles = (n + kTileKeys - 1) / kTileKeys;
    const uint32_t grid = tiles < (uint32_t)kPassGridMax ? tiles : (uint32_t)kPassGridMax;
    if (pass == 0) hipLaunchKernelGGL((k_topk_pass<0, true>), dim3(grid), dim3(kPassThreads), 0, s, sc, key, sel, n, min_count);
    else hipLaunchKernelGGL((k_topk_pass<1, true>), dim3(grid), dim3(kPassThreads), 0, s, sc, key, sel, n, min_count);
    return hipGetLastError();
}

hipError_t launch_topk_select(const TopkScratch& sc, uint32_t k, uint64_t min_count, uint64_t n,
                              uint64_t* top_key, uint64_t* top_count, uint64_t* hdr, hipStream_t s,
                              bool count_selected) {
    hipLaunchKernelGGL(k_topk_compact, dim3(kTopkTableSlots / kCompactChunk), dim3(256), 0, s, sc, min_count);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(k_topk_select, dim3(1), dim3(kSelThreads), 0, s, sc, k, n, top_key, top_count, hdr,
                       count_selected ? 1u : 0u);
    return hipGetLastError();
}

}  // namespace rl
