// The summary / verdict word format of the hot regions (csrc/rl_hot_words.hpp) on the CPU: every
// accessor against the bit positions written out here by hand, round trips at the fields' ends,
// the walk's register form against the stored word, and the chunk / group difference in word 2.
// No engine, no GPU.
#include <cstdint>
#include <cstdio>

#include "../../distributed-rate-limiter_amd/csrc/rl_hot_words.hpp"

using namespace rl::hotw;

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::printf("FAILED %s (%s:%d)\n", #x, __FILE__, __LINE__);     \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static int index_tests() {
    CHECK(kEntryWords == 8 && kVerdictWord == 3);
    CHECK(key_words(0) == 0 && key_words(1) == 4);
    CHECK(rest_word(false) == 3 && rest_word(true) == 7);
    CHECK(rest_word(true) == key_words(1) + kVerdictWord);
    return 0;
}

static int time_tests() {
    // ord_key form (sign bit flipped) back to the signed time; ~0 / 0 mean "no plain acquire"
    CHECK(min_word(~0ULL) == (uint64_t)INT64_MAX && max_word(0ULL) == (uint64_t)INT64_MIN);
    const int64_t ts[] = {0, 1, -1, 1700000000000LL, INT64_MAX - 1, INT64_MIN + 1};
    for (int64_t t : ts) {
        const uint64_t ord = (uint64_t)t ^ 0x8000000000000000ULL;
        CHECK((int64_t)min_word(ord) == t && (int64_t)max_word(ord) == t);
    }
    // the ends of the ordered form are the "none" values themselves
    CHECK(min_word(0ULL) == (uint64_t)INT64_MIN && max_word(~0ULL) == (uint64_t)INT64_MAX);
    return 0;
}

static int chunk_word2_tests() {
    // n_special bits 0-7, n_hot 8-15, n_early 16-23, n_rest 24-31
    CHECK(chunk_counts(1, 0, 0, 0) == 0x00000001ULL);
    CHECK(chunk_counts(0, 1, 0, 0) == 0x00000100ULL);
    CHECK(chunk_counts(0, 0, 1, 0) == 0x00010000ULL);
    CHECK(chunk_counts(0, 0, 0, 1) == 0x01000000ULL);
    CHECK(chunk_counts(64, 64, 64, 64) == 0x40404040ULL);
    CHECK(chunk_n_special(0x000000FFULL) == 255 && chunk_n_special(0xFFFFFF00ULL) == 0);
    CHECK(chunk_n_hot(0x0000FF00ULL) == 255 && chunk_n_hot(0xFFFF00FFULL) == 0);
    CHECK(chunk_n_early(0x00FF0000ULL) == 255 && chunk_n_early(0xFF00FFFFULL) == 0);
    CHECK(chunk_n_rest(0xFF000000ULL) == 255 && chunk_n_rest(0x00FFFFFFULL) == 0);
    const uint32_t ends[] = {0, 1, 63, 64};
    for (uint32_t s : ends) for (uint32_t h : ends) for (uint32_t e : ends) for (uint32_t r : ends) {
        const uint64_t w = chunk_counts(s, h, e, r);
        CHECK(w >> 32 == 0);
        CHECK(chunk_n_special(w) == s && chunk_n_hot(w) == h && chunk_n_early(w) == e && chunk_n_rest(w) == r);
    }
    // n_rest is an 8-bit field: 255 is the most it carries, here and through word 3
    CHECK(chunk_n_rest(chunk_counts(0, 0, 0, 255)) == 255 && chunk_n_hot(chunk_counts(0, 0, 0, 255)) == 0);
    return 0;
}

static int group_word2_tests() {
    // flags: special bit 0, hot bit 8, early bit 16; walk flags bits 24-25
    CHECK(kWalkUnordered == 1 && kWalkWide == 2);
    CHECK(group_flags(true, false, false, 0) == 0x00000001ULL);
    CHECK(group_flags(false, true, false, 0) == 0x00000100ULL);
    CHECK(group_flags(false, false, true, 0) == 0x00010000ULL);
    CHECK(group_flags(false, false, false, kWalkUnordered) == 0x01000000ULL);
    CHECK(group_flags(false, false, false, kWalkWide) == 0x02000000ULL);
    CHECK(group_flags(true, true, true, 3) == 0x03010101ULL);
    for (int m = 0; m < 32; ++m) {
        const bool s = m & 1, h = m & 2, e = m & 4;
        const uint32_t wf = (uint32_t)m >> 3;
        const uint64_t w = group_flags(s, h, e, wf);
        CHECK(group_has_special(w) == s && group_has_hot(w) == h && group_has_early(w) == e);
        CHECK(group_walk_flags(w) == wf);
    }
    // the same bits mean different things at the two levels: a chunk's n_rest must not read as
    // walk flags' absence or presence by accident, nor the flags as a rest count
    CHECK(group_walk_flags(chunk_counts(0, 5, 0, 64)) == 0);      // 64 = bit 30: outside the flags
    CHECK(group_walk_flags(chunk_counts(0, 5, 0, 3)) == 3);       // (why chunk words never go through it)
    CHECK(chunk_n_rest(group_flags(false, true, false, kWalkWide)) == 2);
    // the three leading fields read alike at both levels
    CHECK(group_has_hot(chunk_counts(0, 64, 0, 0)) && !group_has_hot(chunk_counts(64, 0, 64, 64)));
    CHECK(group_has_special(chunk_counts(64, 0, 0, 0)) && group_has_early(chunk_counts(0, 0, 64, 0)));
    return 0;
}

static int word3_tests() {
    // as k_hot_summ leaves it: n_rest << 8
    CHECK(rest_only(0) == 0 && rest_only(1) == 0x100ULL && rest_only(64) == 0x4000ULL && rest_only(255) == 0xFF00ULL);
    CHECK(verdict_n_rest(0xFF00ULL) == 255 && verdict_n_rest(~0xFF00ULL) == 0);
    CHECK(group_has_rest(0x100ULL) && !group_has_rest(~0x100ULL));
    CHECK(!verdict_decided(rest_only(255)) && !verdict_walked(rest_only(255)));
    // the flag bits
    CHECK(kDecided == 1 && kEarly == 2 && kWalked == 4 && kAllows == 8);
    CHECK(verdict_decided(1) && !verdict_decided(~1ULL));
    CHECK(verdict_walked(4) && !verdict_walked(~4ULL));
    CHECK(verdict_plain(1) && verdict_plain(3) && verdict_plain(0xFF03ULL) && !verdict_plain(5) && !verdict_plain(0) && !verdict_plain(4));
    CHECK(verdict_whole_chunk(1) && !verdict_whole_chunk(3) && !verdict_whole_chunk(0x101ULL) &&
          !verdict_whole_chunk(0x8001ULL) && !verdict_whole_chunk(0));
    // threshold verdicts: 1 / 3, n_rest in bits 8-15
    const uint32_t rests[] = {0, 1, 64, 255};
    for (uint32_t r : rests) {
        CHECK(threshold_verdict(r, false) == (((uint64_t)r << 8) | 1u));
        CHECK(threshold_verdict(r, true) == (((uint64_t)r << 8) | 3u));
        CHECK(verdict_n_rest(threshold_verdict(r, true)) == r && verdict_allows(threshold_verdict(r, true)) == 0);
        // walk denial: decided | walked, no allows
        CHECK(walk_denial(r) == (((uint64_t)r << 8) | 5u));
        CHECK(verdict_walked(walk_denial(r)) && verdict_decided(walk_denial(r)) && verdict_allows(walk_denial(r)) == 0);
        CHECK(verdict_n_rest(walk_denial(r)) == r);
    }
    // the group verdict keeps bits 8-15 of the word it replaces, and nothing else of it
    CHECK(group_verdict(0x100ULL, false) == 0x101ULL && group_verdict(0x100ULL, true) == 0x103ULL);
    CHECK(group_verdict(0, false) == 1 && group_verdict(~0ULL, true) == 0xFF03ULL);
    // k_hot_fill's view of a chunk under a decided group
    CHECK(group_decision(0x103ULL) == 3 && group_decision(0x101ULL) == 1 && group_decision(~0ULL) == 3);
    CHECK(with_rest_of(1, 0x4005ULL) == 0x4001ULL && with_rest_of(3, ~0ULL) == 0xFF03ULL);
    return 0;
}

static int allow_tests() {
    // walk verdict with allows: 13 | (count - 1) << 4 | n_rest << 8 | offsets from bit 16, 6 bits each
    CHECK(reg_threshold(false) == 1 && reg_threshold(true) == 3 && reg_walk_denied() == 5);
    CHECK(reg_walk_allows(1, 0) == 13u && reg_walk_allows(4, 0) == (13u | (3u << 4)));
    for (uint32_t count = 1; count <= 4; ++count) {
        for (uint32_t pos = 0; pos < count; ++pos) {
            const uint32_t ends[] = {0, 63};
            for (uint32_t o : ends) {
                // offset o in position pos, 21 (a middle value) in the others
                uint32_t offs = 0;
                for (uint32_t k = 0; k < count; ++k) offs = reg_offsets_add(offs, k, k == pos ? o : 21u);
                uint64_t want = 13u | ((uint64_t)(count - 1) << 4) | (200ULL << 8);
                for (uint32_t k = 0; k < count; ++k) want |= (uint64_t)(k == pos ? o : 21u) << (16 + 6 * k);
                const uint64_t v = walk_allows_verdict(200, count, offs);
                CHECK(v == want);
                CHECK(verdict_decided(v) && verdict_walked(v) && !verdict_plain(v));
                CHECK(verdict_allows(v) == count && verdict_n_rest(v) == 200);
                for (uint32_t k = 0; k < count; ++k) CHECK(verdict_offset(v, k) == (k == pos ? o : 21u));
                CHECK(v >> 40 == 0);
            }
        }
    }
    // every offset at its maximum: bits 16-39 all set, nothing above
    uint32_t offs = 0;
    for (uint32_t k = 0; k < 4; ++k) offs = reg_offsets_add(offs, k, 63u);
    CHECK(offs == 0xFFFFFFu);
    CHECK(walk_allows_verdict(255, 4, offs) == 0xFFFFFFFF3DULL);
    CHECK(reg_offsets_add(0, 0, 63) == 63u && reg_offsets_add(0, 3, 63) == (63u << 18));
    // allows are counted only under bit 3
    CHECK(verdict_allows(0x35ULL) == 0 && verdict_allows(0x3DULL) == 4 && verdict_allows(0x0DULL) == 1);
    return 0;
}

// the conversion of the walk's register form as its flush has always stored it: the flags'
// low byte, the chunk's n_rest from its counts word, the offsets moved up by eight bits
static uint64_t flush_word(uint32_t vF, uint32_t b_w2) {
    return (uint64_t)(vF & 0xFFu) | ((uint64_t)((b_w2 >> 24) & 0xFFu) << 8) | ((uint64_t)(vF >> 8) << 16);
}

static int reg_tests() {
    const uint32_t w2s[] = {0x00000100u, 0x40004001u, 0xFF010203u};
    for (uint32_t b_w2 : w2s) {
        const uint32_t n_rest = chunk_n_rest(b_w2);
        const uint32_t regs[] = {reg_threshold(false), reg_threshold(true), reg_walk_denied(),
                                 reg_walk_allows(1, 63u), reg_walk_allows(2, 5u | (63u << 6)),
                                 reg_walk_allows(4, 0xFFFFFFu), 13u | (3u << 4) | (0xABCDEFu << 8)};
        for (uint32_t vF : regs) CHECK(reg_to_word(vF, n_rest) == flush_word(vF, b_w2));
        CHECK(reg_to_word(reg_threshold(true), n_rest) == threshold_verdict(n_rest, true));
        CHECK(reg_to_word(reg_walk_denied(), n_rest) == walk_denial(n_rest));
    }
    // the literal forms the walk used: 13 | (pc - 1) << 4 | pofs << 8, offsets 6 bits per allow
    for (uint32_t pc = 1; pc <= 4; ++pc) {
        const uint32_t pofs = 0x2Au | (0x15u << 6);
        CHECK(reg_walk_allows(pc, pofs) == (13u | ((pc - 1u) << 4) | (pofs << 8)));
    }
    return 0;
}

int main() {
    if (index_tests() || time_tests() || chunk_word2_tests() || group_word2_tests() || word3_tests() ||
        allow_tests() || reg_tests())
        return 1;
    std::printf("hot words: ok\n");
    return 0;
}
