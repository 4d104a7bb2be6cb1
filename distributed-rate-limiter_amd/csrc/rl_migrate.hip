// rl_migrate.hip — key migration: copy or drop the state of a listed set of keys, bit for bit
// (rl_copy_keys / rl_drop_keys, include/rl_engine.h). The insert side, rl_put_keys, is the
// state import's region rebuild with the cache word carried (k_import, rl_state.hip).
//
// The work is one lookup per (key, limiter) pair: pair p = key p / n_lim under limiter
// p % n_lim, at most 8192 x 255 pairs per launch. Four lanes look one pair up with the quad
// probe of rl_table.hpp, bucket by bucket from the key's home. A hit is emitted iff the slot
// holds state or a cache word (slot_holds_state, the rule growth and import keep); tombstones
// and absent keys emit nothing. No `now` is involved: state that is dead by TTL travels as it
// is. Hits are compacted through one counter with one atomic per wave; the host sorts them.
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
#include "rl_table.hpp"

namespace rl {

constexpr int kMoveThreads = 256;
constexpr uint32_t kMoveBlockPairs = kMoveThreads / 4;

template <bool DROP>
__global__ __launch_bounds__(kMoveThreads) void k_move_keys(MoveArgs a) {
    const uint32_t lane = threadIdx.x & 63, sub = lane & 3;
    const uint64_t n_pairs = (uint64_t)a.n_keys * a.n_lim;
    const uint64_t p = ((uint64_t)blockIdx.x * kMoveThreads + threadIdx.x) >> 2;   // this quad's pair
    bool op = p < n_pairs;                          // still probing
    uint64_t key = 0, h = 0;
    uint32_t lim = 0;
    int algo = 0;
    TableRegion R{nullptr, nullptr};                // the key's region (and its cache words)
    if (op) {
        key = a.key[p / a.n_lim];
        lim = (uint32_t)(p % a.n_lim);
        h = mix64(key);
        const DevLimiter& L = a.lims[lim];
        algo = L.algo;
        R = table_region(L, h, a.shard_bits);
    }
    QuadSlot v{{0, 0}, {0, 0}, 0};
    uint32_t pos = 0;                               // < kRegionSlots: inside the region
    bool mine = false;                              // this lane holds the key's slot
    // (wave-uniform trip count; nearly always one. A full region without the key: absent)
    for (uint32_t m = 0; m < kProbeBuckets; ++m) {
        if (op) {
            pos = quad_pos(h, m, sub);
            v = quad_load(R, pos);
        }
        quad_resolve(op, v, h, lane, mine);
        if (!__any(op)) break;
    }
    // ---- the hits, compacted: one atomic per wave
    const bool emit = mine && slot_holds_state(algo, Slot{v.lo.x, v.lo.y, v.hi.x, v.hi.y}, v.x);
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
        im.word[0] = v.lo.y; im.word[1] = v.hi.x; im.word[2] = v.hi.y;
        im.cache_word = v.x;
        im.limiter = (uint16_t)lim;
        a.out[idx] = im;
    }
    if constexpr (DROP) {
        const Slot t = slot_used(Slot{h, 0, 0, 0});                // tag 0: c = kDeadMark
        RL_GLOBAL u64x2_t* sp = (RL_GLOBAL u64x2_t*)(R.tab + pos);
        sp[0] = u64x2_t{t.tag, t.a};
        sp[1] = u64x2_t{t.b, t.c};
        if (R.xtab) R.xtab[pos] = 0;
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
