// Mixed operations and retry-after queries through the multi-GPU router (rl_router_execute,
// rl_router_retry_after, include/rl_engine.h). The ranks are threads of one process on one
// GPU over the in-process transport (loop_transport.hpp), each with its own engine shard.
//
// Reference: ONE unsharded engine in the same process, given the ranks' slices concatenated in
// rank order through rl_execute_batch_device, step after step, and every rank's queries
// through rl_retry_after_device at the same point of the stream (after step 2). Every
// allowed / remaining / wait_ms must be equal.
//
//   test_router_query execute  : G = 2, G = 4, split rounds (recv_cap 7000), the wide layout,
//                                a hot-key directory, op without limiter ids, and a plain
//                                rl_router_step (op = NULL) beside them
//   test_router_query retry    : the queries again with a small recv_cap, the wide layout, the
//                                directory, and without limiter ids
//   test_router_query mismatch : routers with different max_batch
//   test_router_query shards   : G = 8, operations and queries in split rounds, with and without
//                                the directory
// Every case runs 3 steps, 3 query calls per rank (the last step's own arrays with
// skip = allowed; crafted queries; a layout with one empty rank and one rank all skipped), a
// 4th step and rl_router_finish. A counting wrapper around the transport checks the number of
// all_to_all_v calls and the bytes sent.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rl_engine.h"
#include "loop_transport.hpp"

static int failures = 0;
#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) {                                                                   \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                               \
        }                                                                             \
    } while (0)
#define HIPC(x) CHECK((x) == hipSuccess)

static uint64_t mix(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27; x *= 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}
static double u01(uint64_t x) { return (double)(mix(x) >> 11) * 0x1.0p-53; }

static const int64_t NS = 1000000, T0 = 1700000000000LL;
static const int64_t kFar = ((int64_t)1 << 31) + 5;           // ms: past the compact wire's range
static const int kSteps = 4, kQuerySets = 3;
static const size_t kN = 20000, kNQ = 3000, kKeys = 5000;
static const int64_t kLims[2][3] = {{1, 50, 60000}, {0, 30, 5000}};   // TB 50 @ 10/s, SW 30 / 5 s
static const double kRefill[2] = {10.0, 0.0};

struct Cfg {
    const char* what;
    int G;
    size_t recv_cap;
    bool wide, dir, no_limiter, plain;     // plain: rl_router_step, no operations
};

struct Reqs {                               // request or query arrays (host)
    std::vector<uint64_t> key;
    std::vector<int32_t> permits;
    std::vector<int64_t> now;
    std::vector<uint16_t> lim;
    std::vector<uint8_t> op;                // operations, or a query's skip mask
    bool has_skip = false;
    size_t n() const { return key.size(); }
};

static uint64_t key_of(uint64_t zipf_rank) { return mix(zipf_rank + 0x5EED0000ULL); }

// Zipf-1.2 over kKeys by inversion of the cumulative weights
static std::vector<double> zipf_cdf() {
    std::vector<double> c(kKeys);
    double s = 0;
    for (size_t k = 0; k < kKeys; ++k) { s += std::pow((double)(k + 1), -1.2); c[k] = s; }
    for (double& x : c) x /= s;
    return c;
}

// The global stream: request ((st * G + rank) * kN + i). About 90 % acquire, 7 % peek, 3 %
// reset; a handful of op = 3, permits = 0 and limiter ids 300, 0x3FFF, 0x4001.
static Reqs make_trace(const Cfg& c) {
    static const std::vector<double> cdf = zipf_cdf();
    const size_t total = (size_t)kSteps * c.G * kN;
    Reqs t;
    for (size_t i = 0; i < total; ++i) {
        const uint64_t rank = (uint64_t)(std::lower_bound(cdf.begin(), cdf.end(), u01(i * 3 + 1)) - cdf.begin());
        t.key.push_back(key_of(rank));
        t.permits.push_back(1 + (int32_t)(mix(i * 3 + 2) % 4));
        t.now.push_back((T0 + (int64_t)((double)i * 40000.0 / (double)total)) * NS + (int64_t)(mix(i) % NS));
        t.lim.push_back(c.no_limiter ? 0 : (uint16_t)(rank % 2));
        const double u = u01(i * 3 + 3);
        t.op.push_back(c.plain ? 0 : (u < 0.90 ? RL_OP_ACQUIRE : (u < 0.97 ? RL_OP_PEEK : RL_OP_RESET)));
        switch (i % 9973) {
        case 1: if (!c.plain) t.op[i] = 3; break;
        case 2: t.permits[i] = 0; break;
        case 3: if (!c.no_limiter) t.lim[i] = 300; break;
        case 4: if (!c.no_limiter) t.lim[i] = 0x3FFF; break;
        case 5: if (!c.no_limiter) t.lim[i] = 0x4001; break;
        case 6: if (!c.plain) t.op[i] = 255; break;
        default: break;
        }
    }
    if (c.wide) {                           // step 1, rank 0: one request far after the slice's first
        const size_t b = ((size_t)1 * c.G + 0) * kN;
        t.key[b + 100] = mix(0xFEEDULL);
        t.now[b + 100] = t.now[b] + kFar * NS;
    }
    return t;
}

// Query set `which` of `rank` (asked after step 2). 0: the last step's own requests with
// skip = its allowed output (`allowed`: the step's decisions for this rank). 1: crafted: seen,
// unseen and duplicate keys, permits 0 and > max, limiter 300. 2: rank 0 asks nothing, rank 1
// skips everything, the others skip every second query.
static Reqs make_queries(const Cfg& c, const Reqs& tr, int rank, int which, const uint8_t* allowed) {
    Reqs q;
    if (which == 0) {
        const size_t b = ((size_t)2 * c.G + rank) * kN;
        q.key.assign(tr.key.begin() + b, tr.key.begin() + b + kN);
        q.permits.assign(tr.permits.begin() + b, tr.permits.begin() + b + kN);
        q.now.assign(tr.now.begin() + b, tr.now.begin() + b + kN);
        q.lim.assign(tr.lim.begin() + b, tr.lim.begin() + b + kN);
        q.op.assign(allowed, allowed + kN);
        q.has_skip = true;
        return q;
    }
    if (which == 2 && rank == 0) return q;
    const int64_t tend = T0 + 30000 + 100 * rank;             // the end of step 2, in ms
    for (size_t i = 0; i < kNQ; ++i) {
        uint64_t zr = mix(i + 77 * (uint64_t)rank) % 50;
        uint64_t key = key_of(zr);
        int32_t p = 1 + (int32_t)(i % 4);
        uint16_t lim = (uint16_t)(zr % 2);
        switch (i % 6) {
        case 1: key = mix(0xABCD0000ULL + i + 100000 * (uint64_t)rank); lim = (uint16_t)(i % 2); break;   // unseen
        case 2: key = key_of(0); lim = 0; p = 3; break;                                                     // duplicates
        case 3: p = 0; break;
        case 4: p = 1000; break;
        case 5: if (!c.no_limiter) lim = 300; break;
        default: break;
        }
        q.key.push_back(key);
        q.permits.push_back(p);
        q.now.push_back((tend + (int64_t)(i % 1000)) * NS + (int64_t)(mix(i) % NS));
        q.lim.push_back(c.no_limiter ? 0 : lim);
        q.op.push_back(which == 2 ? (rank == 1 ? 1 : (uint8_t)(i % 2)) : 0);
    }
    q.has_skip = which == 2;
    if (c.wide && which == 1 && rank == 2 % c.G) q.now[7] = q.now[0] + kFar * NS;
    return q;
}

static size_t live_of(const Reqs& q) {
    size_t l = 0;
    for (size_t i = 0; i < q.n(); ++i) l += !(q.has_skip && q.op[i]);
    return l;
}

// ---- device arrays of one request / query batch
struct Dev {
    uint64_t* k; int32_t* p; int64_t* t; uint16_t* l; uint8_t* o; uint8_t* a; int64_t* r;
    explicit Dev(size_t n) {
        n = std::max<size_t>(n, 1);
        HIPC(hipMalloc((void**)&k, n * 8)); HIPC(hipMalloc((void**)&p, n * 4)); HIPC(hipMalloc((void**)&t, n * 8));
        HIPC(hipMalloc((void**)&l, n * 2)); HIPC(hipMalloc((void**)&o, n)); HIPC(hipMalloc((void**)&a, n));
        HIPC(hipMalloc((void**)&r, n * 8));
    }
    ~Dev() {
        HIPC(hipFree(k)); HIPC(hipFree(p)); HIPC(hipFree(t)); HIPC(hipFree(l)); HIPC(hipFree(o));
        HIPC(hipFree(a)); HIPC(hipFree(r));
    }
    void load(const Reqs& q, size_t b, size_t n, hipStream_t s) {
        if (!n) return;
        HIPC(hipMemcpyAsync(k, &q.key[b], n * 8, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(p, &q.permits[b], n * 4, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(t, &q.now[b], n * 8, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(l, &q.lim[b], n * 2, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(o, &q.op[b], n, hipMemcpyHostToDevice, s));
    }
};

// max_skew_ms: a step spans 10 s of trace time and a rank asks about its own slice afterwards, so
// a query's now lies up to 10 s before the end of the stream the engines have seen. Split rounds
// are separate engine batches, each with a later earliest request than the one batch the
// reference runs for the whole step; without the allowance an owner may drop a bucket that is
// dead at a later round's earliest request and still in the reference's table (both read it as
// expired from then on, but a query at an earlier now would see it). rl_opts.max_skew_ms is the
// engine's contract for timestamps that lag behind earlier batches; every engine here, the
// reference included, gets the same 15 s.
static rl_engine* make_engine(uint64_t max_batch, uint32_t shard, uint32_t shards) {
    rl_opts o{};
    o.device = 0; o.max_batch = max_batch; o.default_capacity = (uint64_t)1 << 16;
    o.max_skew_ms = 15000;
    o.shard_index = shard; o.shard_count = shards;
    rl_engine* e = nullptr;
    CHECK(rl_create(&o, &e) == RL_OK);
    for (int l = 0; l < 2; ++l) {
        rl_limiter_config c{};
        c.algo = (int)kLims[l][0]; c.max_permits = kLims[l][1]; c.window_ms = kLims[l][2];
        c.refill_per_s = kRefill[l]; c.capacity = (uint64_t)1 << 16;
        uint16_t id;
        CHECK(rl_add_limiter_ex(e, &c, &id) == RL_OK && id == l);
    }
    return e;
}

struct Answers {                            // decisions of the 4 steps and waits of the 3 query sets
    std::vector<uint8_t> a;
    std::vector<int64_t> r;
    std::vector<int64_t> w[kQuerySets];
};

// ---- the reference: one engine, the concatenated stream
static void reference(const Cfg& c, const Reqs& tr, std::vector<Answers>* want, int* finish) {
    const int G = c.G;
    const size_t n = (size_t)G * kN;
    rl_engine* e = make_engine(n, 0, 1);
    if (c.wide) CHECK(rl_tune(e, "wide_records", 1) == RL_OK);   // (every setting decides alike)
    hipStream_t s;
    HIPC(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    Dev d(n);
    int64_t* dw;
    HIPC(hipMalloc((void**)&dw, kN * 8));
    std::vector<uint8_t> a(n);
    std::vector<int64_t> r(n);
    for (int rank = 0; rank < G; ++rank) { (*want)[rank].a.resize(kSteps * kN); (*want)[rank].r.resize(kSteps * kN); }
    *finish = RL_OK;
    for (int st = 0; st < kSteps; ++st) {
        d.load(tr, (size_t)st * n, n, s);
        CHECK(rl_execute_batch_device(e, n, d.k, d.p, d.t, c.no_limiter ? nullptr : d.l, c.plain ? nullptr : d.o,
                                      d.a, d.r, nullptr, s) == RL_OK);
        HIPC(hipMemcpyAsync(a.data(), d.a, n, hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(r.data(), d.r, n * 8, hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        const int rc = rl_last_status(e);
        CHECK(rc == RL_OK || rc == RL_E_INVALID_REQUEST);
        if (rc != RL_OK) *finish = rc;
        for (int rank = 0; rank < G; ++rank) {
            std::copy(a.begin() + rank * kN, a.begin() + (rank + 1) * kN, (*want)[rank].a.begin() + st * kN);
            std::copy(r.begin() + rank * kN, r.begin() + (rank + 1) * kN, (*want)[rank].r.begin() + st * kN);
        }
        if (st != 2) continue;
        for (int rank = 0; rank < G; ++rank)
            for (int which = 0; which < kQuerySets; ++which) {
                const Reqs q = make_queries(c, tr, rank, which, &(*want)[rank].a[2 * kN]);
                (*want)[rank].w[which].assign(q.n(), 12345);
                if (!q.n()) continue;
                d.load(q, 0, q.n(), s);
                CHECK(rl_retry_after_device(e, q.n(), d.k, d.p, d.t, c.no_limiter ? nullptr : d.l,
                                            q.has_skip ? d.o : nullptr, dw, s) == RL_OK);
                HIPC(hipMemcpyAsync((*want)[rank].w[which].data(), dw, q.n() * 8, hipMemcpyDeviceToHost, s));
                HIPC(hipStreamSynchronize(s));
            }
    }
    HIPC(hipFree(dw));
    HIPC(hipStreamDestroy(s));
    rl_destroy(e);
}

// ---- the counting transport
struct Counting {
    looptest::Endpoint ep;
    int world;
    std::vector<uint64_t> log;              // bytes sent by every all_to_all_v call
};
static int counting_a2av(void* ctx, const void* send, const uint64_t* so, const uint64_t* sb, void* recv,
                         const uint64_t* ro, const uint64_t* rb, void* stream) {
    Counting* c = (Counting*)ctx;
    uint64_t sent = 0;
    for (int p = 0; p < c->world; ++p) sent += sb[p];
    c->log.push_back(sent);
    return looptest::all_to_all_v(&c->ep, send, so, sb, recv, ro, rb, stream);
}

struct RankOut {
    Answers got;
    int finish = 0;
    uint64_t travelled[kQuerySets] = {0, 0, 0};     // query bytes without the header and status rows
    size_t query_calls[kQuerySets] = {0, 0, 0};
};

static bool same_stats(const rl_batch_stats& x, const rl_batch_stats& y) {
    return std::memcmp(&x, &y, sizeof(x)) == 0;
}

static void run_rank(const Cfg* cp, int rank, looptest::Hub* hub, const Reqs* trp, RankOut* out) {
    const Cfg& c = *cp;
    const Reqs& tr = *trp;
    const int G = c.G;
    HIPC(hipSetDevice(0));
    rl_engine* e = make_engine((uint64_t)G * kN, (uint32_t)rank, (uint32_t)G);
    Counting ct{{hub, rank}, G, {}};
    rl_transport t{&ct, counting_a2av};
    rl_router* r = nullptr;
    rl_router_opts ro{};
    ro.max_batch = kN; ro.recv_cap = c.recv_cap;
    CHECK(rl_router_create_ex(e, (uint32_t)G, (uint32_t)rank, &t, &ro, &r) == RL_OK);
    hipStream_t s;
    HIPC(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    Dev d(kN), dq(kNQ);
    int64_t* dw;
    HIPC(hipMalloc((void**)&dw, kN * 8));
    if (c.dir) {                            // the hottest keys of this rank's whole slice as candidates
        std::map<uint64_t, uint64_t> cnt;
        for (int st = 0; st < kSteps; ++st)
            for (size_t i = 0; i < kN; ++i) cnt[tr.key[((size_t)st * G + rank) * kN + i]]++;
        std::vector<std::pair<uint64_t, uint64_t>> v(cnt.begin(), cnt.end());
        std::sort(v.begin(), v.end(), [](auto& x, auto& y) { return x.second > y.second || (x.second == y.second && x.first < y.first); });
        v.resize(std::min<size_t>(v.size(), 64));
        std::vector<uint64_t> k, n;
        for (auto& x : v) { k.push_back(x.first); n.push_back(x.second); }
        uint32_t placed = 0;
        CHECK(rl_router_plan_directory(r, k.size(), k.data(), n.data(), (uint64_t)kSteps * kN, 16, &placed, s) == RL_OK);
        CHECK(placed == 16);
    }
    out->got.a.resize(kSteps * kN);
    out->got.r.resize(kSteps * kN);
    const uint16_t* lim = c.no_limiter ? nullptr : d.l;
    auto step = [&](int st) {
        rl_router_stats s0{}, s1{};
        CHECK(rl_router_stats_get(r, &s0) == RL_OK);
        d.load(tr, ((size_t)st * G + rank) * kN, kN, s);
        ct.log.clear();
        const int rc = c.plain ? rl_router_step(r, kN, d.k, d.p, d.t, lim, d.a, d.r, s)
                               : rl_router_execute(r, kN, d.k, d.p, d.t, lim, d.o, d.a, d.r, s);
        CHECK(rc == RL_OK);
        HIPC(hipMemcpyAsync(&out->got.a[st * kN], d.a, kN, hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(&out->got.r[st * kN], d.r, kN * 8, hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        CHECK(rl_router_stats_get(r, &s1) == RL_OK);
        CHECK(s1.steps == s0.steps + 1);
        // the collectives of a step with limiter ids, with or without op: header, then per
        // round the payload (1 compact / 3 wide), the u16 column and the return trip
        const uint64_t rounds = s1.rounds - s0.rounds;
        const bool col = !c.no_limiter || !c.plain, wide_step = c.wide && st == 1;
        CHECK(col);
        if (c.recv_cap) CHECK(rounds > 1); else CHECK(rounds == 1);
        const size_t want_calls = 1 + rounds * ((wide_step ? 3 : 1) + 1 + 1);
        CHECK(ct.log.size() == want_calls);
        if (!wide_step && ct.log.size() >= 3) {
            if (rounds == 1) {              // 16 + 2 B per request forward
                CHECK(ct.log[1] == 16 * kN && ct.log[2] == 2 * kN);
            } else {
                uint64_t w = 0, l = 0;
                for (uint64_t k = 0; k < rounds; ++k) { w += ct.log[1 + 3 * k]; l += ct.log[2 + 3 * k]; }
                CHECK(w == 16 * kN && l == 2 * kN);
            }
        }
    };
    for (int st = 0; st < 3; ++st) step(st);
    // ---- the queries, between steps
    rl_batch_stats b0{}, b1{};
    rl_router_stats r0{}, r1{};
    CHECK(rl_batch_stats_get(e, &b0) == RL_OK);
    CHECK(rl_router_stats_get(r, &r0) == RL_OK);
    for (int which = 0; which < kQuerySets; ++which) {
        const Reqs q = make_queries(c, tr, rank, which, &out->got.a[2 * kN]);
        const size_t n = q.n();
        int rc;
        ct.log.clear();
        HIPC(hipMemsetAsync(dw, 0x5A, kN * 8, s));
        if (which == 0) {                   // the step's own device arrays and its allowed output
            rc = rl_router_retry_after(r, kN, d.k, d.p, d.t, lim, d.a, dw, s);
        } else {
            dq.load(q, 0, n, s);
            rc = rl_router_retry_after(r, n, dq.k, dq.p, dq.t, c.no_limiter ? nullptr : dq.l,
                                       q.has_skip ? dq.o : nullptr, dw, s);
        }
        CHECK(rc == RL_OK);
        out->got.w[which].assign(n, 777);
        if (n) HIPC(hipMemcpy(out->got.w[which].data(), dw, n * 8, hipMemcpyDeviceToHost));   // (the call was synchronous)
        out->query_calls[which] = ct.log.size();
        CHECK(ct.log.size() >= 4);
        for (size_t k = 1; k + 1 < ct.log.size(); ++k) out->travelled[which] += ct.log[k];
        if (ct.log.size() >= 2) {
            CHECK(ct.log.back() == 8 * (uint64_t)G);           // the status row
            CHECK(ct.log.front() % (8 * (uint64_t)G) == 0);    // the header rows
        }
    }
    CHECK(rl_batch_stats_get(e, &b1) == RL_OK);
    CHECK(rl_router_stats_get(r, &r1) == RL_OK);
    CHECK(same_stats(b0, b1));
    CHECK(r1.steps == r0.steps && r1.rounds == r0.rounds && r1.split_steps == r0.split_steps &&
          r1.max_recv == r0.max_recv);
    step(3);
    out->finish = rl_router_finish(r);
    rl_router_destroy(r);
    HIPC(hipFree(dw));
    HIPC(hipStreamDestroy(s));
    rl_destroy(e);
}

static void run_case(const Cfg& c) {
    const int G = c.G;
    const Reqs tr = make_trace(c);
    std::vector<Answers> want(G);
    int want_finish = 0;
    reference(c, tr, &want, &want_finish);
    looptest::Hub hub(G);
    std::vector<RankOut> out(G);
    std::vector<std::thread> th;
    for (int rank = 0; rank < G; ++rank) th.emplace_back(run_rank, &c, rank, &hub, &tr, &out[rank]);
    for (auto& x : th) x.join();
    size_t bad = 0, badw = 0, denied = 0, special = 0, nz = 0;
    uint64_t live[kQuerySets] = {0, 0, 0}, travelled[kQuerySets] = {0, 0, 0};
    for (int rank = 0; rank < G; ++rank) {
        CHECK(out[rank].finish == want_finish);
        for (size_t i = 0; i < (size_t)kSteps * kN; ++i) {
            if (out[rank].got.a[i] != want[rank].a[i] || out[rank].got.r[i] != want[rank].r[i]) {
                if (bad < 3)
                    std::fprintf(stderr, "%s: rank %d request %zu: got (%d,%lld) want (%d,%lld)\n", c.what, rank, i,
                                 out[rank].got.a[i], (long long)out[rank].got.r[i], want[rank].a[i],
                                 (long long)want[rank].r[i]);
                ++bad;
            }
            denied += !want[rank].a[i];
        }
        for (int which = 0; which < kQuerySets; ++which) {
            // the router's skip mask for set 0 is its own allowed output: equal to the
            // reference's when the decisions above are
            const Reqs q = make_queries(c, tr, rank, which, &want[rank].a[2 * kN]);
            live[which] += live_of(q);
            travelled[which] += out[rank].travelled[which];
            CHECK(out[rank].got.w[which].size() == want[rank].w[which].size());
            CHECK(out[rank].query_calls[which] == out[0].query_calls[which]);
            for (size_t i = 0; i < q.n() && i < out[rank].got.w[which].size(); ++i) {
                const int64_t g = out[rank].got.w[which][i], w = want[rank].w[which][i];
                if (g != w) {
                    if (badw < 3)
                        std::fprintf(stderr, "%s: rank %d set %d query %zu: wait %lld want %lld\n", c.what, rank,
                                     which, i, (long long)g, (long long)w);
                    ++badw;
                }
                if (q.has_skip && q.op[i]) CHECK(g == 0);
                special += w == RL_RETRY_NEVER || w == RL_RETRY_INVALID;
                nz += w > 0;
            }
        }
    }
    CHECK(bad == 0);
    CHECK(badw == 0);
    CHECK(want_finish == RL_E_INVALID_REQUEST);        // the stream holds invalid requests
    CHECK(denied > 0 && nz > 0 && special > 0);          // the trace reaches every kind of answer
    // what travelled: per live query 16 + 2 B forward (8 + 4 + 8 + 2 in the wide layout) and 8 B back
    for (int which = 0; which < kQuerySets; ++which) {
        const bool wide_q = c.wide && which == 1;
        const uint64_t ids = c.no_limiter ? 0 : 1;
        const uint64_t fwd = (wide_q ? 20 : 16) + 2 * ids;
        CHECK(travelled[which] == (fwd + 8) * live[which]);
        const size_t per_round = (wide_q ? 4 : 2) + ids;
        CHECK((out[0].query_calls[which] - 2) % per_round == 0);
        if (c.recv_cap && which == 0) CHECK(out[0].query_calls[which] > 2 + per_round);   // several rounds
    }
    CHECK(live[2] < live[1]);
    std::printf("%s: %zu requests, %zu mismatches; queries live %llu / %llu / %llu, %zu wait mismatches, "
                "%zu all_to_all_v calls for set 0\n",
                c.what, (size_t)kSteps * G * kN, bad, (unsigned long long)live[0], (unsigned long long)live[1],
                (unsigned long long)live[2], badw, out[0].query_calls[0]);
}

// Routers with different max_batch: seen by every rank in the header; every rank returns
// RL_E_INVALID_ARG and all of its waits read RL_RETRY_ERROR.
static void mismatch_case() {
    const int G = 2;
    const size_t n = 1000;
    looptest::Hub hub(G);
    std::vector<int> rc(G, 0);
    std::vector<std::vector<int64_t>> w(G);
    std::vector<std::thread> th;
    for (int rank = 0; rank < G; ++rank)
        th.emplace_back([&, rank] {
            HIPC(hipSetDevice(0));
            rl_engine* e = make_engine(8 * n, (uint32_t)rank, (uint32_t)G);
            looptest::Endpoint ep{&hub, rank};
            rl_transport t = looptest::transport(&ep);
            rl_router* r = nullptr;
            rl_router_opts ro{};
            ro.max_batch = n + 16 * (size_t)rank; ro.recv_cap = 2 * n;
            CHECK(rl_router_create_ex(e, (uint32_t)G, (uint32_t)rank, &t, &ro, &r) == RL_OK);
            Dev d(n);
            Reqs q;
            for (size_t i = 0; i < n; ++i) {
                q.key.push_back(key_of(i)); q.permits.push_back(1); q.now.push_back(T0 * NS);
                q.lim.push_back(0); q.op.push_back((uint8_t)(i % 2));
            }
            d.load(q, 0, n, nullptr);
            HIPC(hipDeviceSynchronize());
            rc[rank] = rl_router_retry_after(r, n, d.k, d.p, d.t, d.l, d.o, d.r, nullptr);
            w[rank].assign(n, 0);
            HIPC(hipMemcpy(w[rank].data(), d.r, n * 8, hipMemcpyDeviceToHost));
            CHECK(rl_router_retry_after(r, n + 17, d.k, d.p, d.t, d.l, d.o, d.r, nullptr) == RL_E_TOO_LARGE);
            CHECK(rl_router_retry_after(r, n, nullptr, d.p, d.t, d.l, d.o, d.r, nullptr) == RL_E_INVALID_ARG);
            CHECK(rl_router_retry_after(r, n, d.k, d.p, d.t, d.l, d.o, nullptr, nullptr) == RL_E_INVALID_ARG);
            rl_router_destroy(r);
            rl_destroy(e);
        });
    for (auto& x : th) x.join();
    for (int rank = 0; rank < G; ++rank) {
        CHECK(rc[rank] == RL_E_INVALID_ARG);
        size_t err = 0;
        for (int64_t x : w[rank]) err += x == RL_RETRY_ERROR;
        CHECK(err == n);
    }
    std::printf("capacity mismatch: every rank returned %d %d\n", rc[0], rc[1]);
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "execute";
    //                what                           G  recv_cap wide   dir    no_lim plain
    const Cfg exec[] = {{"G=2 ops", 2, 0, false, false, false, false},
                        {"G=4 ops", 4, 0, false, false, false, false},
                        {"G=4 ops, split rounds (recv_cap 7000)", 4, 7000, false, false, false, false},
                        {"G=4 ops, wide layout", 4, 0, true, false, false, false},
                        {"G=4 ops, hot-key directory", 4, 0, false, true, false, false},
                        {"G=4 ops without limiter ids", 4, 0, false, false, true, false},
                        {"G=4 plain step (op = NULL)", 4, 0, false, false, false, true}};
    const Cfg retry[] = {{"G=4 queries, recv_cap 3000", 4, 3000, false, false, false, false},
                         {"G=4 queries, wide + recv_cap 7000", 4, 7000, true, false, false, false},
                         {"G=4 queries, directory + recv_cap 7000", 4, 7000, false, true, false, false},
                         {"G=2 queries without limiter ids", 2, 0, false, false, true, false}};
    // G = 8: the Zipf-1.2 trace's first key draws a fifth of all requests, 1.7 n of the 8 n of a
    // step, so its owner receives more than the default capacity of 2 n: both cases state a
    // receive capacity and every step runs in rounds
    const Cfg shards[] = {{"G=8 ops, split rounds (recv_cap 7000)", 8, 7000, false, false, false, false},
                          {"G=8 queries, directory + recv_cap 7000", 8, 7000, false, true, false, false}};
    if (mode == "shards") {
        for (const Cfg& c : shards) run_case(c);
    } else if (mode == "execute") {
        for (const Cfg& c : exec) run_case(c);
    } else if (mode == "retry") {
        for (const Cfg& c : retry) run_case(c);
    } else if (mode == "mismatch") {
        mismatch_case();
    } else {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    std::printf("%s: %s (%d failures)\n", mode.c_str(), failures ? "FAIL" : "ok", failures);
    return failures ? 1 : 0;
}
