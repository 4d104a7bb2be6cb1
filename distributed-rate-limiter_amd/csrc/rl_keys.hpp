// rl_keys.hpp — the arithmetic of a string-key batch (rl_key_hash, rl_hash_keys,
// rl_execute_batch_keys; kernel in rl_keys.hip, host side in rl_engine_query.cpp).
// Plain C++ with no HIP header, so tests/cpp/test_keys_plan.cpp checks it on the CPU against
// brute force; the kernel and the engine call the same functions.
//
// A batch is key_bytes[key_bytes_len] plus key_off[n + 1]; key i is the bytes
// [key_off[i], key_off[i + 1]). Two rules live here.
//  * Well-formed: key i is well-formed iff key_off[i] <= key_off[i + 1] <= key_bytes_len and
//    key_off[i + 1] - key_off[i] <= kKeyMaxBytes. The host forms refuse a batch with a
//    malformed key; the device form hashes it to 0 without reading a byte of it.
//  * The chunk: the host forms stage a batch whose keys are all well-formed (so its offsets do
//    not decrease) in chunks cut at key boundaries. The chunk that starts at key `at` holds the
//    largest m >= 1 with m <= max_keys, at + m <= n and key_off[at + m] - key_off[at] <=
//    max_bytes; max_bytes >= kKeyMaxBytes, so m = 1 always fits and every chunk makes progress.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RL_KEYS_HD __host__ __device__
#else
#define RL_KEYS_HD
#endif

namespace rl {

constexpr uint64_t kKeyMaxBytes = 4096;                  // RL_KEY_MAX_BYTES
constexpr uint64_t kFnvOffset = 0xcbf29ce484222325ULL;   // FNV-1a 64
constexpr uint64_t kFnvPrime = 0x100000001b3ULL;         // = 2^40 + 0x1b3

// Offsets are taken relative to a chunk's first byte by the caller (o - bias, wrapping): an
// offset below the bias wraps to a huge value and fails one of the first two comparisons.
RL_KEYS_HD inline bool key_well_formed(uint64_t o0, uint64_t o1, uint64_t bytes_len) {
    return o0 <= o1 && o1 <= bytes_len && o1 - o0 <= kKeyMaxBytes;
}

// The first malformed key of the batch, or n if every key is well-formed.
inline size_t keys_first_malformed(const uint64_t* off, size_t n, uint64_t bytes_len) {
    for (size_t i = 0; i < n; ++i)
        if (!key_well_formed(off[i], off[i + 1], bytes_len)) return i;
    return n;
}

// Keys of the chunk that starts at key `at` (< n) of a batch without malformed keys.
inline size_t keys_chunk(const uint64_t* off, size_t n, size_t at, size_t max_keys, uint64_t max_bytes) {
    size_t hi = n - at < max_keys ? n - at : max_keys;   // m <= hi
    size_t lo = 1;                                       // m = lo fits
    const uint64_t base = off[at];
    while (lo < hi) {                                    // offsets do not decrease: bisect
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (off[at + mid] - base <= max_bytes) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace rl
