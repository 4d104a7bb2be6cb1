// rl_hot_words.hpp — the summary / verdict words of the hot regions: the whole interface between
// k_hot_summ (writes them), the chains (rewrite them as verdicts) and k_hot_fill / walk_fill_key
// (read them). The only place that knows the layout; plain constexpr functions, no HIP include
// (tests/cpp/test_hot_words.cpp checks every bit position on the CPU).
//
// Eight 64-bit words per chunk (64 records, hot_summ) and per group (64 chunks, hot_summ2),
// four per key: the dominant key's at 0, the second key's at 4 (key_words).
//
//   word 0  min time of the key's plain acquires      (INT64_MAX: none)
//   word 1  max time of the key's plain acquires      (INT64_MIN: none)
//   word 2  chunk: n_special | n_hot << 8 | n_early << 16 | n_rest << 24 (counts of the key's peeks /
//                  resets, of its records, of its TB acquires above max_permits, and of the
//                  records of other keys)
//           group: the same three leading counts as 0/1 flags over the group's chunks, and in
//                  bits 24-25 the walk flags: the key's plain acquires are not in time order
//                  (kWalkUnordered) or ask for more than 2 permits (kWalkWide); either keeps
//                  the chain off the allow walk. (A group's rest flag lives in word 3 only.)
//   word 3  as k_hot_summ leaves it: n_rest << 8 (group: the 0/1 flag). n_rest counts the
//           records of other keys: for the dominant key every other record, for the second
//           key those of neither (the records pass 2 applies); with no second key the second
//           key's word repeats the dominant key's count, so rest_word names the word to read.
//           As a verdict (a chain decided the key's records of the chunk / group; words 0-2
//           then hold the key's state a, b, c under which they are decided):
//             bit 0       decided
//             bit 1       TB early rejects (permits > max) among the records
//             bit 2       an allow walk's verdict (chunk level only)
//             bit 3       the walk allowed some of the records
//             bits 4-5    their count - 1 (1..4)
//             bits 8-15   n_rest, carried through
//             bits 16-39  the allowed records' offsets in the chunk, 6 bits each, ascending
//           Every record of the key is denied under the state but the allowed ones; the records
//           after each allow are judged under the state that allow leaves.
//
// The walk keeps a chunk's pending verdict in a 32-bit register form (vF): the flag bits 0-7 as
// stored, the offsets from bit 8 on; reg_to_word puts n_rest back between them.
#pragma once
#include <cstdint>

namespace rl {
namespace hotw {

constexpr uint32_t kEntryWords = 8;                     // per chunk / group
constexpr uint32_t key_words(uint32_t k) { return 4u * k; }
constexpr uint32_t kVerdictWord = 3;                   // of a key's four
// the verdict word whose n_rest counts the records of no chained key
constexpr uint32_t rest_word(bool second_key) { return second_key ? 7u : 3u; }

// ---- words 0 / 1: from the order-preserving unsigned form (ord_key); ~0 / 0: no plain acquire
constexpr uint64_t kSign = 0x8000000000000000ULL;
constexpr uint64_t min_word(uint64_t ord_min) { return ord_min == ~0ULL ? (uint64_t)INT64_MAX : ord_min ^ kSign; }
constexpr uint64_t max_word(uint64_t ord_max) { return ord_max == 0ULL ? (uint64_t)INT64_MIN : ord_max ^ kSign; }

// ---- word 2 of a chunk
constexpr uint64_t chunk_counts(uint32_t n_special, uint32_t n_hot, uint32_t n_early, uint32_t n_rest) {
    return n_special | (n_hot << 8) | (n_early << 16) | (n_rest << 24);
}
constexpr uint32_t chunk_n_special(uint64_t w2) { return (uint32_t)w2 & 0xFFu; }
constexpr uint32_t chunk_n_hot(uint64_t w2) { return ((uint32_t)w2 >> 8) & 0xFFu; }
constexpr uint32_t chunk_n_early(uint64_t w2) { return ((uint32_t)w2 >> 16) & 0xFFu; }
constexpr uint32_t chunk_n_rest(uint64_t w2) { return (uint32_t)(w2 >> 24) & 0xFFu; }

// ---- word 2 of a group
constexpr uint32_t kWalkUnordered = 1u, kWalkWide = 2u;
constexpr uint64_t group_flags(bool special, bool hot, bool early, uint32_t walk_flags) {
    return (special ? 1u : 0u) | ((hot ? 1u : 0u) << 8) | ((early ? 1u : 0u) << 16) | ((uint64_t)walk_flags << 24);
}
constexpr bool group_has_special(uint64_t w2) { return ((uint32_t)w2 & 0xFFu) != 0u; }
constexpr bool group_has_hot(uint64_t w2) { return (((uint32_t)w2 >> 8) & 0xFFu) != 0u; }
constexpr bool group_has_early(uint64_t w2) { return (((uint32_t)w2 >> 16) & 0xFFu) != 0u; }
constexpr uint32_t group_walk_flags(uint64_t w2) { return ((uint32_t)w2 >> 24) & 3u; }

// ---- word 3 as k_hot_summ leaves it, and n_rest in either form
constexpr uint64_t rest_only(uint64_t n_rest) { return n_rest << 8; }
constexpr uint32_t verdict_n_rest(uint64_t w3) { return (uint32_t)(w3 >> 8) & 0xFFu; }
constexpr bool group_has_rest(uint64_t w3) { return ((w3 >> 8) & 1u) != 0u; }

// ---- word 3 as a verdict
constexpr uint32_t kDecided = 1u, kEarly = 2u, kWalked = 4u, kAllows = 8u;
constexpr bool verdict_decided(uint64_t v) { return (v & kDecided) != 0u; }
constexpr bool verdict_walked(uint64_t v) { return (v & kWalked) != 0u; }
constexpr bool verdict_plain(uint64_t v) { return (v & (kDecided | kWalked)) == kDecided; }
// decided, and every record of the chunk is this key's plain acquire: no read needed
constexpr bool verdict_whole_chunk(uint64_t v) { return (v & kDecided) && !(v & (0xFF00u | kEarly)); }
constexpr uint32_t verdict_allows(uint64_t v) { return (v & kAllows) ? (uint32_t)((v >> 4) & 3u) + 1u : 0u; }
constexpr uint32_t verdict_offset(uint64_t v, uint32_t k) { return (uint32_t)(v >> (16 + 6 * k)) & 63u; }

// the register form: the three verdict kinds that occur
constexpr uint32_t reg_threshold(bool early) { return early ? (kDecided | kEarly) : kDecided; }
constexpr uint32_t reg_walk_denied() { return kDecided | kWalked; }
constexpr uint32_t reg_walk_allows(uint32_t count, uint32_t offs) {            // count 1..4
    return (kDecided | kWalked | kAllows) | ((count - 1u) << 4) | (offs << 8);
}
constexpr uint32_t reg_offsets_add(uint32_t offs, uint32_t count, uint32_t off) { return offs | (off << (6 * count)); }
constexpr uint64_t reg_to_word(uint32_t vF, uint32_t n_rest) {
    return (uint64_t)(vF & 0xFFu) | ((uint64_t)n_rest << 8) | ((uint64_t)(vF >> 8) << 16);
}
// the stored forms
constexpr uint64_t threshold_verdict(uint32_t n_rest, bool early) { return ((uint64_t)n_rest << 8) | reg_threshold(early); }
constexpr uint64_t walk_denial(uint32_t n_rest) { return reg_to_word(reg_walk_denied(), n_rest); }
constexpr uint64_t walk_allows_verdict(uint32_t n_rest, uint32_t count, uint32_t offs) {
    return reg_to_word(reg_walk_allows(count, offs), n_rest);
}
// a group decided by the thresholds: its rest flag stays
constexpr uint64_t group_verdict(uint64_t w3, bool early) { return (w3 & 0xFF00u) | reg_threshold(early); }
// k_hot_fill: a chunk's verdict when its group is decided as a whole (the group's decision,
// the chunk's own n_rest)
constexpr uint64_t group_decision(uint64_t group_w3) { return group_w3 & (kDecided | kEarly); }
constexpr uint64_t with_rest_of(uint64_t v, uint64_t chunk_w3) { return v | (chunk_w3 & 0xFF00u); }

}  // namespace hotw
}  // namespace rl
