// rl_migrate.hip — key migration: copy or drop the state of a listed set of keys, bit for bit
// (rl_copy_keys / rl_drop_keys, include/rl_engine.h). The insert side, rl_put_keys, is the
// state import's region rebuild with the cache word carried (k_import, rl_misc.hip).
//
// The work is one lookup per (key, limiter) pair: pair p = key p / n_lim under limiter
// p % n_lim, at most 8192 x 255 pairs per launch. Four lanes look one pair up, as
// k_retry_after does: each lane loads one 32-B slot of the key's 4-slot bucket as two 16-B
// loads (a probe step of a pair is one 128-B line) plus its cache word, the quad finds the
// matching or the first free slot from the wave's ballots, and the probe walks on bucket by
// bucket from slot_home until either shows up (rl_device.hpp: a key sits before the first free
// slot of its probe sequence). A hit is emitted iff the slot holds state or a cache word, the
// rule k_grow / k_import keep; tombstones and absent keys emit nothing. No `now` is involved:
// state that is dead by TTL travels as it is. Hits are compacted through one counter with one
// atomic per wave; the host sorts them.
//
// Drop: the lane that holds the hit rewrites its slot as a tombstone with plain vector stores
// (tag kept, state words zero through slot_used, cache word zero). The host hands over distinct
// keys, so distinct pairs never share a slot and nobody else writes it. A drop never frees a
// slot: the tag stays in the slot's first 16 bytes, so whatever mix of old and new words a
// concurrent probe of the same region reads, it sees a used slot that is not its own and walks
// on; the probe chains stay valid while the launch runs and afterwards (no free slot appears
// inside a chain). The one tag that is zero (key_hash 0: mix64(0) == 0) relies on kDeadMark in
// the second 16 bytes instead, and a probe could read that half old and the rest new; the host
// therefore drops key 0 in a launch of its own, in which each pair probes a different
// limiter's table.
#include "rl_kcommon.hpp"

namespace rl {

constexpr int kMoveThreads = 256;
constexpr uint32_t kMoveBlockPairs = kMoveThreads / 4;

typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));

template <bool DROP>
__global__ __launch_bounds__(kMoveThreads) void k_move_keys(MoveArgs a) {
    const uint32_t lane = threadIdx.x & 63, sub = lane & 3, qbase = lane & ~3u;
    const uint64_t n_pairs = (uint64_t)a.n_keys * a.n_lim;
    const uint64_t p = ((uint64_t)blockIdx.x * kMoveThreads + threadIdx.x) >> 2;   // this quad's pair
    bool op = p < n_pairs;                          // still probing
    uint64_t key = 0, h = 0;
    uint32_t lim = 0;
    int algo = 0;
    RL_GLOBAL Slot* tab = nullptr;                  // the key's region (and its cache words)
    RL_GLOBAL uint64_t* xtab = nullptr;
    if (op) {
        key = a.key[p / a.n_lim];
        lim = (uint32_t)(p % a.n_lim);
        h = mix64(key);
        const DevLimiter& L = a.lims[lim];
        algo = L.algo;
        const size_t r0 = (size_t)region_local(h, a.shard_bits, L.region_bits) * kRegionSlots;
        tab = as_global((Slot*)L.table + r0);
        xtab = L.cache_table ? as_global((uint64_t*)L.cache_table + r0) : nullptr;
    }
    const uint32_t home = slot_home(h);
    u64x2_t lo{0, 0}, hi{0, 0};
    uint64_t x = 0;
    uint32_t pos = 0;                               // < kRegionSlots: inside the region
    bool mine = false;                              // this lane holds the key's slot
    // (wave-uniform trip count; nearly always one. A full region without the key: absent)
    for (uint32_t m = 0; m < kRegionSlots / 4; ++m) {
        bool match = false, isfree = false;
        if (op) {
            pos = (home + 4 * m + sub) & (kRegionSlots - 1);
            RL_GLOBAL const u64x2_t* sp = (RL_GLOBAL const u64x2_t*)(tab + pos);
            lo = sp[0]; hi = sp[1];
            x = xtab ? xtab[pos] : 0;
            isfree = (lo.x | lo.y | hi.x | hi.y | x) == 0;
            match = !isfree && lo.x == h;
        }
        const uint32_t qm = (uint32_t)(__ballot(match) >> qbase) & 0xFu;
        const uint32_t qf = (uint32_t)(__ballot(isfree) >> qbase) & 0xFu;
        if (op && (qm | qf)) {
            // a match after a free slot of the same bucket cannot be the key's (invariant)
            const bool found = qm != 0 && (qf == 0 || __builtin_ctz(qm) < __builtin_ctz(qf));
            mine = found && match && sub == (uint32_t)__builtin_ctz(qm);
            op = false;
        }
        if (!__any(op)) break;
    }
    // ---- the hits, compacted: one atomic per wave
    const bool emit = mine && (x != 0 || state_present(algo, hi.x, hi.y));
    const uint64_t em = __ballot(emit);
    if (em == 0) return;                            // (wave-uniform)
    const int leader = __builtin_ctzll(em);
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(a.count, (uint32_t)__builtin_popcountll(em));
    base = (uint32_t)__shfl((int)base, leader, 64);
    if (!emit) return;
    const uint32_t idx = base + popc_below(em);
    if (idx < a.cap) {
        KeyImage im{};
        im.key_hash = key;
        im.word[0] = lo.y; im.word[1] = hi.x; im.word[2] = hi.y;
        im.cache_word = x;
        im.limiter = (uint16_t)lim;
        a.out[idx] = im;
    }
    if constexpr (DROP) {
        const Slot t = slot_used(Slot{h, 0, 0, 0});                // tag 0: c = kDeadMark
        RL_GLOBAL u64x2_t* sp = (RL_GLOBAL u64x2_t*)(tab + pos);
        sp[0] = u64x2_t{t.tag, t.a};
        sp[1] = u64x2_t{t.b, t.c};
        if (xtab) xtab[pos] = 0;
    }
}

hipError_t launch_move_keys(const MoveArgs& a, bool drop, hipStream_t s) {
    const uint64_t n_pairs = (uint64_t)a.n_keys * a.n_lim;
    if (n_pairs == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)((n_pairs + kMoveBlockPairs - 1) / kMoveBlockPairs);
    if (drop) hipLaunchKernelGGL(k_move_keys<true>, dim3(grid), dim3(kMoveThreads), 0, s, a);
    else hipLaunchKernelGGL(k_move_keys<false>, dim3(grid), dim3(kMoveThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace rl
