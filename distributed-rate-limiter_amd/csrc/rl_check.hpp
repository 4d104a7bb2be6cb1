// rl_check.hpp — the rules a limiter's table must satisfy (rl_check_limiter, rl_check_images;
// include/rl_engine.h; DESIGN.md §4 "Checking a table"). Plain C++ with no HIP header, so
// tests/cpp/test_check_plan.cpp checks every predicate on the CPU against brute force; the kernel
// (rl_check.hip) calls the same functions.
//
// The rules are those of the HBM slot invariant (above slot_free, rl_device.hpp), read as a
// checker and not as a writer. They apply to region r of a table with k region bits, the
// engine's shard bits and kCheckRegionSlots slots per region; a slot is USED iff its four words
// and its cache word are not all zero.
//
// Structural classes (whatever wrote the table):
//   WRONG_REGION  a used slot whose tag does not hash to region r (check_region_of). Shard
//                 ownership is not checked: the owner directory moves keys between shards.
//   UNREACHABLE   a used slot s with a free slot in the cyclic range [home(tag), s): exactly when
//                 the quad probe (quad_resolve, rl_table.hpp) stops before s and reports the key
//                 absent. A region with no free slot has none.
//   DUPLICATE     a used slot whose tag also sits in a used slot of the region with a lower
//                 index, where both copies hold bucket state and neither was dead before the
//                 other was last written (n such copies count n - 1). Two slots with one tag are
//                 not corruption by themselves: a batch never hits a tombstone and an insert
//                 claims the FIRST tombstone of its chain (rl_region.hpp, the probe of
//                 apply_group), so a key that comes back after its TTL may claim another key's
//                 dead slot and leave its own dead slot, tag and all, further down the chain.
//                 Such a stale copy expired before the region load that made the new one
//                 (keep_from, rl_kcommon.hpp) and every write of the new one is later:
//                 last_write(stale) + ttl < last_write(new), ttl = w (SW) / 2w (TB). Copies that
//                 are not ordered like that claim the key at the same time, which no writer does.
//   DEAD_MARK     token bucket only: c == kCheckDeadMark on a slot other than {tag 0, a 0, b 0}
//                 with a zero cache word, the one slot slot_used (rl_device.hpp) writes it to. (A
//                 sliding-window slot keeps two offsets in c, and c == 2 is "last INCR 2 ms into
//                 the newest bucket, older offset 0": ordinary state, so no rule.)
// Value classes (state no entry point can produce from inputs it accepts):
//   SW_START      state present (b != 0) and b1_start % w != 0: sw_geo (rl_device.hpp) gives
//                 curr_start = q * w, and rl_import_state refuses window_start_ms % w != 0.
//   SW_OFFSET     a bucket with a non-zero count whose last_off is outside (-w, w). sw_step_g
//                 stores now - curr_start, and curr_start = trunc(now / w) * w (jdiv truncates as
//                 Java does), so now < 0 gives offsets in (-w, 0] and now >= 0 in [0, w);
//                 rl_import_state admits [0, w). Offsets of zero-count buckets are unconstrained:
//                 a reset leaves them stale.
//   TB_FLAGS      token bucket: c has bits other than bit 0 and is not kCheckDeadMark (tb_step
//                 writes 1 or 0, rl_import_state 1, slot_used the mark).
// Two classes the ids of which stay reserved are NOT checked, because rl_import_state admits
// what the decision code cannot write (rl_engine_state.cpp): SW_COUNT (a bucket count above
// max_permits: import takes any count in [1, 2^32)) and TB_TOKENS (a balance that is NaN,
// infinite, negative or above capacity: import takes the double as it comes). Their counters
// read 0 and their first positions ~0.
// Image lists (rl_check_images) take the value classes, per image with its limiter's constants,
// and two classes of their own: IMAGE_LIMITER (the engine has no such limiter; the value classes
// are then skipped) and IMAGE_RESERVED (a non-zero reserved field).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RL_CHECK_HD __host__ __device__
#else
#define RL_CHECK_HD
#endif

namespace rl {

constexpr uint32_t kCheckRegionSlots = 256;       // kRegionSlots
constexpr uint32_t kCheckClasses = 16;            // RL_CHECK_CLASSES
constexpr uint64_t kCheckDeadMark = 2;            // kDeadMark
constexpr int kCheckAlgoSW = 0, kCheckAlgoTB = 1; // kAlgoSW, kAlgoTB
constexpr uint64_t kCheckNone = ~0ULL;            // first[]: no such slot
constexpr uint64_t kCheckMaxImages = 1ull << 31;

// class ids (RL_CHECK_*, include/rl_engine.h)
enum : uint32_t {
    kCkWrongRegion = 0, kCkUnreachable = 1, kCkDuplicate = 2, kCkDeadMark = 3,
    kCkSwStart = 4, kCkSwCount = 5 /* reserved */, kCkSwOffset = 6, kCkTbFlags = 7,
    kCkTbTokens = 8 /* reserved */, kCkImageLimiter = 9, kCkImageReserved = 10,
};

// What the value classes need of a limiter.
struct CheckLimiter {
    int32_t algo;
    int64_t window_ms;       // 0 < w < 2^31
    int64_t ttl_ms;          // SW: w, TB: 2w (DevLimiter::ttl_ms)
};

// ------------------------------------------------------------------ a slot on its own
RL_CHECK_HD inline bool check_used(uint64_t tag, uint64_t a, uint64_t b, uint64_t c, uint64_t x) {
    return (tag | a | b | c | x) != 0;
}
// state_present / slot_holds_state (rl_device.hpp, rl_table.hpp): what a snapshot emits
RL_CHECK_HD inline bool check_holds_state(int algo, uint64_t b, uint64_t c, uint64_t x) {
    return x != 0 || (algo == kCheckAlgoTB ? (c & 1u) != 0 : b != 0);
}
// region_local (rl_device.hpp): the k bits of the tag below the shard bits
RL_CHECK_HD inline uint32_t check_region_of(uint64_t tag, int shard_bits, int k) {
    if (k == 0) return 0;
    return (uint32_t)((tag << shard_bits) >> (64 - k));
}
// slot_home (rl_kcommon.hpp): the first slot of the tag's probe sequence, 4-aligned
RL_CHECK_HD inline uint32_t check_home(uint64_t tag) { return (uint32_t)tag & (kCheckRegionSlots - 4); }

// The value classes of one slot (or image) as a bit per class id; structural bit kCkDeadMark too,
// since it needs the slot's words only.
RL_CHECK_HD inline uint32_t check_slot_values(const CheckLimiter& L, uint64_t tag, uint64_t a, uint64_t b,
                                              uint64_t c, uint64_t x) {
    uint32_t m = 0;
    if (L.algo == kCheckAlgoTB) {
        if (c == kCheckDeadMark) {
            if ((tag | a | b | x) != 0) m |= 1u << kCkDeadMark;
        } else if (c & ~(uint64_t)1) {
            m |= 1u << kCkTbFlags;
        }
        return m;
    }
    const int64_t w = L.window_ms;
    const uint32_t c1 = (uint32_t)b, c0 = (uint32_t)(b >> 32);
    const int64_t o1 = (int32_t)(uint32_t)c, o0 = (int32_t)(uint32_t)(c >> 32);
    if (b != 0 && (int64_t)a % w != 0) m |= 1u << kCkSwStart;
    if ((c1 != 0 && (o1 <= -w || o1 >= w)) || (c0 != 0 && (o0 <= -w || o0 >= w))) m |= 1u << kCkSwOffset;
    return m;
}

// The time of a slot's last write, if it holds bucket state (*lw): TB the last refill; SW the
// newest last-INCR time over its buckets with a count. Wrapping arithmetic: garbage words give a
// garbage time, never undefined behaviour.
RL_CHECK_HD inline bool check_last_write(const CheckLimiter& L, uint64_t a, uint64_t b, uint64_t c, int64_t* lw) {
    if (L.algo == kCheckAlgoTB) {
        *lw = (int64_t)b;
        return (c & 1u) != 0;
    }
    const uint32_t c1 = (uint32_t)b, c0 = (uint32_t)(b >> 32);
    const int64_t t1 = (int64_t)(a + (uint64_t)(int64_t)(int32_t)(uint32_t)c);
    const int64_t t0 = (int64_t)(a - (uint64_t)L.window_ms + (uint64_t)(int64_t)(int32_t)(uint32_t)(c >> 32));
    *lw = c1 != 0 && (c0 == 0 || t1 >= t0) ? t1 : t0;
    return b != 0;
}
// Two copies of one tag that both hold bucket state conflict unless one had expired before the
// other was last written.
RL_CHECK_HD inline bool check_copies_conflict(int64_t lw_x, int64_t lw_y, int64_t ttl) {
    const __int128 x = lw_x, y = lw_y, t = ttl;
    return !(x + t < y) && !(y + t < x);
}

// ------------------------------------------------------------------ a slot in its region
// The free map of a region: bit (s & 63) of word s >> 6 is set iff slot s is free.
struct CheckFreeMap { uint64_t w[kCheckRegionSlots / 64]; };

RL_CHECK_HD inline uint64_t check_bits_below(uint32_t n) {        // bits [0, n), n <= 64
    return n >= 64 ? ~0ULL : ((1ULL << n) - 1);
}
// Any free slot in [lo, hi), 0 <= lo <= hi <= kCheckRegionSlots: mask arithmetic, no loop over slots.
RL_CHECK_HD inline bool check_free_in(const CheckFreeMap& F, uint32_t lo, uint32_t hi) {
    uint64_t any = 0;
    for (uint32_t j = 0; j < kCheckRegionSlots / 64; ++j) {
        const uint32_t base = j * 64;
        const uint32_t l = lo <= base ? 0u : (lo - base >= 64 ? 64u : lo - base);
        const uint32_t h = hi <= base ? 0u : (hi - base >= 64 ? 64u : hi - base);
        any |= F.w[j] & check_bits_below(h) & ~check_bits_below(l);
    }
    return any != 0;
}
// A used slot s whose key the probe cannot reach: a free slot in the cyclic range [home, s).
RL_CHECK_HD inline bool check_unreachable(const CheckFreeMap& F, uint64_t tag, uint32_t s) {
    const uint32_t home = check_home(tag);
    s &= kCheckRegionSlots - 1;
    if (home <= s) return check_free_in(F, home, s);
    return check_free_in(F, home, kCheckRegionSlots) || check_free_in(F, 0, s);
}

// first[] position of slot s of region r
RL_CHECK_HD inline uint64_t check_pos(uint64_t region, uint32_t s) {
    return region << 8 | (s & (kCheckRegionSlots - 1));
}

}  // namespace rl
