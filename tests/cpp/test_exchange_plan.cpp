// The round plan of a router exchange (distributed-rate-limiter_amd/csrc/rl_exchange.hpp)
// against brute force, on the CPU: for G in {1, 2, 4, 8}, random count matrices (zero rows and
// columns included) and receive capacities 1, one that divides an owner's stream evenly and one
// that does not, every owner's stream is written out request by request (sources in rank
// order), cut into pieces of `cap`, and compared with what every rank's plan sends and expects.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../distributed-rate-limiter_amd/csrc/rl_exchange.hpp"

using namespace rl;

static int failures = 0;
#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) {                                                                   \
            if (failures < 20)                                                        \
                std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                               \
        }                                                                             \
    } while (0)

static uint64_t mix(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27; x *= 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

static void check(const std::vector<uint64_t>& C, uint32_t G, uint64_t cap) {
    // brute force: owner o's stream, one (source, index in the source's segment for o) per request
    std::vector<std::vector<std::pair<uint32_t, uint64_t>>> stream(G);
    uint64_t want_rounds = 1;
    for (uint32_t o = 0; o < G; ++o) {
        for (uint32_t p = 0; p < G; ++p)
            for (uint64_t i = 0; i < C[(size_t)p * G + o]; ++i) stream[o].push_back({p, i});
        want_rounds = std::max<uint64_t>(want_rounds, (stream[o].size() + cap - 1) / cap);
    }
    std::vector<ExchangePlan> plan;
    for (uint32_t p = 0; p < G; ++p) plan.push_back(exchange_plan(C, G, p, cap));
    std::vector<uint64_t> next((size_t)G * G, 0);      // next[p][o]: first of p's requests for o not yet sent
    for (uint32_t p = 0; p < G; ++p) {
        CHECK(plan[p].rounds == want_rounds);
        CHECK(plan[p].m == stream[p].size());
        uint64_t seg = 0;
        for (uint32_t o = 0; o < G; ++o) {
            CHECK(plan[p].counts[o] == C[(size_t)p * G + o] && plan[p].rc[o] == C[(size_t)o * G + p]);
            CHECK(plan[p].seg[o] == seg);
            seg += plan[p].counts[o];
        }
    }
    for (uint64_t k = 0; k < want_rounds; ++k) {
        std::vector<ExchangeRound> R;
        for (uint32_t p = 0; p < G; ++p) R.push_back(exchange_round(plan[p], k));
        for (uint32_t o = 0; o < G; ++o) {
            // what o expects: at most cap, sources in rank order from offset 0
            uint64_t at = 0;
            for (uint32_t p = 0; p < G; ++p) {
                CHECK(R[o].ro[p] == at);
                at += R[o].rr[p];
            }
            CHECK(R[o].mk == at && at <= cap);
            const uint64_t lo = std::min<uint64_t>(k * cap, stream[o].size());
            const uint64_t hi = std::min<uint64_t>((k + 1) * cap, stream[o].size());
            CHECK(at == hi - lo);                       // piece k of o's stream, whole
            for (uint32_t p = 0; p < G; ++p) {
                // what p sends to o is what o expects from p ...
                CHECK(R[p].sc[o] == R[o].rr[p]);
                // ... the next requests of p's segment for o, in order, each range once
                const uint64_t beg = R[p].so[o] - plan[p].seg[o];
                CHECK(R[p].sc[o] == 0 || beg == next[(size_t)p * G + o]);
                CHECK(R[p].so[o] >= plan[p].seg[o] && beg + R[p].sc[o] <= C[(size_t)p * G + o]);
                // ... and they are the stream's requests at the positions where o stores them
                for (uint64_t j = 0; j < R[p].sc[o]; ++j) {
                    const uint64_t pos = lo + R[o].ro[p] + j;
                    CHECK(pos < hi && stream[o][pos].first == p && stream[o][pos].second == beg + j);
                }
                next[(size_t)p * G + o] += R[p].sc[o];
            }
        }
    }
    for (size_t i = 0; i < C.size(); ++i) CHECK(next[i] == C[i]);   // covered exactly once
    // a round past the last one moves nothing
    for (uint32_t p = 0; p < G; ++p) CHECK(exchange_round(plan[p], want_rounds).mk == 0);
}

int main() {
    size_t cases = 0;
    for (uint32_t G : {1u, 2u, 4u, 8u})
        for (uint64_t seed = 0; seed < 40; ++seed) {
            std::vector<uint64_t> C((size_t)G * G);
            const uint64_t zero_row = seed % 3 == 0 ? mix(seed) % G : G;
            const uint64_t zero_col = seed % 4 == 0 ? mix(seed + 99) % G : G;
            for (uint32_t p = 0; p < G; ++p)
                for (uint32_t o = 0; o < G; ++o) {
                    uint64_t c = mix(seed * 1000 + p * 16 + o + G) % 23;
                    if (mix(seed + p * 7 + o) % 5 == 0) c = 0;
                    if (p == zero_row || o == zero_col || seed == 1) c = 0;   // seed 1: nothing at all
                    C[(size_t)p * G + o] = c;
                }
            uint64_t m0 = 0, mmax = 0;
            for (uint32_t o = 0; o < G; ++o) {
                uint64_t mo = 0;
                for (uint32_t p = 0; p < G; ++p) mo += C[(size_t)p * G + o];
                if (o == 0) m0 = mo;
                mmax = std::max(mmax, mo);
            }
            // 1; a divisor of owner 0's stream (2 pieces when it is even); one that divides
            // nothing evenly; exactly the largest stream; more than any stream
            std::vector<uint64_t> caps = {1, m0 >= 2 && m0 % 2 == 0 ? m0 / 2 : std::max<uint64_t>(m0, 1),
                                          7, std::max<uint64_t>(mmax, 1), mmax + 5};
            for (uint64_t cap : caps) { check(C, G, cap); ++cases; }
        }
    std::printf("exchange plan: %zu cases, %s (%d failures)\n", cases, failures ? "FAIL" : "ok", failures);
    return failures ? 1 : 0;
}
