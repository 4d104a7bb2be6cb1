// rl_exchange.hpp — the host-only arithmetic of a router exchange (rl_router_step /
// rl_router_execute / rl_router_retry_after, rl_router.cpp): from the count matrix
// C[src][owner] that every rank reads out of the header rows, the receive capacity and this
// rank, the number of rounds and each round's per-pair send and receive ranges. Every rank
// derives its side of the same plan, so what p sends to o in a round is what o expects from p.
// Plain C++ (no HIP), so tests/cpp/test_exchange_plan.cpp checks it on the CPU.
//
// Each owner's incoming stream is its sources' segments in rank order (= global arrival
// order); it is cut into pieces of at most `cap` requests and round k moves piece k of every
// owner. A source's requests for owner o sit at seg[o] .. seg[o] + counts[o] of its owner-order
// arrays and at Pm[o] .. of o's stream; an owner stores a round's piece from offset 0 of its
// receive buffers, sources in rank order.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace rl {

struct ExchangePlan {
    uint32_t world = 0, me = 0;
    uint64_t cap = 1;                 // requests an owner takes per round
    uint64_t rounds = 1;              // max(1, max over owners of ceil(received / cap))
    uint64_t m = 0;                   // requests this rank receives over all rounds
    std::vector<uint64_t> counts;     // [world] mine to each owner
    std::vector<uint64_t> rc;         // [world] each source's to me
    std::vector<uint64_t> seg;        // [world] first of my requests for owner o (owner order)
    std::vector<uint64_t> Pm;         // [world] my start in owner o's stream
    std::vector<uint64_t> Q;          // [world] source p's start in my stream
};

// One round: element offsets / counts for an all-to-all (send side per owner, receive side per
// source); mk = requests this rank receives in the round (<= cap).
struct ExchangeRound {
    std::vector<uint64_t> so, sc, ro, rr;
    uint64_t mk = 0;
};

// C: world x world, row-major, C[src * world + owner]. cap >= 1.
inline ExchangePlan exchange_plan(const std::vector<uint64_t>& C, uint32_t world, uint32_t me,
                                  uint64_t cap) {
    ExchangePlan P;
    const uint32_t G = world;
    P.world = G; P.me = me; P.cap = std::max<uint64_t>(cap, 1);
    P.counts.assign(G, 0); P.rc.assign(G, 0); P.seg.assign(G, 0); P.Pm.assign(G, 0); P.Q.assign(G, 0);
    for (uint32_t p = 0; p < G; ++p) { P.counts[p] = C[(size_t)me * G + p]; P.rc[p] = C[(size_t)p * G + me]; }
    for (uint32_t o = 0; o < G; ++o) {
        uint64_t mo = 0;
        for (uint32_t p = 0; p < G; ++p) {
            if (p == me) P.Pm[o] = mo;
            mo += C[(size_t)p * G + o];
        }
        P.rounds = std::max<uint64_t>(P.rounds, (mo + P.cap - 1) / P.cap);
        if (o == me) P.m = mo;
    }
    for (uint32_t p = 1; p < G; ++p) {
        P.seg[p] = P.seg[p - 1] + P.counts[p - 1];
        P.Q[p] = P.Q[p - 1] + P.rc[p - 1];
    }
    return P;
}

// The part of [start, start + len) inside the window [lo, hi), relative to start.
inline void exchange_clip(uint64_t lo, uint64_t hi, uint64_t start, uint64_t len, uint64_t* beg,
                          uint64_t* end) {
    auto rel = [&](uint64_t w) { return w <= start ? 0 : std::min(w - start, len); };
    *beg = rel(lo);
    *end = rel(hi);
}

inline ExchangeRound exchange_round(const ExchangePlan& P, uint64_t k) {
    const uint32_t G = P.world;
    ExchangeRound R;
    R.so.assign(G, 0); R.sc.assign(G, 0); R.ro.assign(G, 0); R.rr.assign(G, 0);
    const uint64_t lo = k * P.cap, hi = (k + 1) * P.cap;
    for (uint32_t o = 0; o < G; ++o) {
        uint64_t b, e;
        exchange_clip(lo, hi, P.Pm[o], P.counts[o], &b, &e);
        R.so[o] = P.seg[o] + b;
        R.sc[o] = e - b;
    }
    for (uint32_t p = 0; p < G; ++p) {
        uint64_t b, e;
        exchange_clip(lo, hi, P.Q[p], P.rc[p], &b, &e);
        R.rr[p] = e - b;
        R.ro[p] = R.mk;
        R.mk += R.rr[p];
    }
    return R;
}

}  // namespace rl
