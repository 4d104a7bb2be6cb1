// rl_router.cpp — the multi-GPU router behind include/rl_engine.h (rl_router_*).
//
// One router per GPU; every rank holds a contiguous slice of the global arrival stream
// (rank order). A step moves each request to the shard that owns its key and the decision
// back, with the same protocol as distributed-rate-limiter_amd/python/rl_amd/router.py:
//
//   1. owner partition + compact 16-B wire records       (device, no host round-trip)
//   2. header exchange {count, base_ms, overflow, status, capacities, now range, and the
//      source's count for every owner}; ONE host read of the headers (RCCL takes per-peer
//      byte counts on the host). Every rank then knows the whole count matrix, so all of
//      them derive the same exchange plan: one round, or — when some owner would receive
//      more than its receive capacity — several rounds, each moving the next piece of every
//      owner's incoming stream (sources in rank order, so per-key arrival order holds)
//   3. payload all-to-all (+ the u16 limiter ids when there are several limiters)
//   4. the owner's engine decides (engine_execute_routed: rl_execute_batch_device, always the pipeline)
//   5. decisions back in the engine's packed width, one segment + exception block per
//      source (exact remainders outside the width: TB balances below -3)
//   6. scatter back to the caller's order through the partition permutation
//
// A source whose batch spans more than 2^31 ms either side of its first request sends the
// whole step in the wide SoA layout instead (every rank sees its overflow flag).
// Errors are collective: each rank publishes its engine's status in the next header, so all
// ranks fail at the same step.
// rl_router_execute is that step with an operation per request (rl_router_step: none);
// rl_router_retry_after runs the same exchange for the denials' waits (end of this file). The
// round plan of all three is rl_exchange.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/rl_engine.h"
#include "rl_exchange.hpp"
#include "rl_launch.hpp"
#include "rl_replan.hpp"

using namespace rl;

namespace {
constexpr uint32_t kExcCap = 4096;   // exception entries per (owner, source) pair per step

bool fatal(int64_t st) { return st < 0 && st != RL_E_INVALID_REQUEST; }

// Bytes of a segmented return trip of `total` requests over G segments, any width and split.
uint64_t ret_bound(uint32_t G, uint64_t total) {
    return total * 8 + (uint64_t)G * (8 + ret_block_bytes(kExcCap));
}
// Words of the directory exchange: {n, sampled} rows both ways, this rank's candidates, and
// every rank's candidates.
size_t dir_words(uint32_t G) { return 4 * (size_t)G + 2 * (size_t)kDirMax * (1 + (size_t)G); }

}  // namespace

struct rl_router {
    rl_engine* e = nullptr;
    uint32_t world = 1, rank = 0;
    rl_transport t{};
    size_t cap = 0;                      // largest per-rank n (max_batch); every rank's must match
    size_t rcap = 0;                     // requests an owner decides per exchange round
    hipStream_t own = nullptr;           // used when the caller passes stream = NULL
    hipEvent_t done = nullptr;           // recorded at the end of every step on its stream
    bool stepped = false;                // `done` has been recorded
    // send side (cap); everything below is allocated by rl_router_create, so a step never
    // allocates and no rank can fail alone between two collectives
    uint32_t* perm = nullptr;
    uint64_t* wire_s = nullptr;
    uint16_t* lim_s = nullptr;
    int64_t* hdr2 = nullptr;             // [base_ms, overflow] of this source
    uint64_t* mm_part = nullptr;         // [kWireBlocksMax][2] now_ms min / max partials
    int64_t* hdr = nullptr;              // [2][world][kHdrWords]: sent rows, received rows
    uint64_t* k_s = nullptr;             // wide layout (SoA in owner order)
    int32_t* p_s = nullptr;
    int64_t* t_s = nullptr;
    int64_t* back_w = nullptr;           // 8-B decisions back (wide layout / split steps)
    uint8_t* ret_in = nullptr;
    uint64_t ret_in_cap = 0;
    uint64_t* dir = nullptr;             // directory exchange (dir_words)
    // receive side (rcap)
    uint64_t* wire_r = nullptr;
    uint16_t* lim_r = nullptr;
    uint8_t* op_r = nullptr;             // the operations decoded from lim_r (rl_router_execute)
    uint64_t* k_r = nullptr;
    int32_t* p_r = nullptr;
    int64_t* t_r = nullptr;
    uint8_t* a_r = nullptr;
    int64_t* rem_r = nullptr;
    int64_t* packed_r = nullptr;
    uint8_t* ret_out = nullptr;
    uint64_t ret_out_cap = 0;
    uint32_t* lost = nullptr;
    int64_t* h_hdr = nullptr;            // pinned copy of hdr
    unsigned long long* acc = nullptr;   // split rounds: the rounds' engine statuses, folded on
                                         // device (kStatusAccWords), settled at the next step
    int64_t pub = RL_OK;                 // status this rank publishes in the next header
    int64_t held = RL_OK;                // a step's status settled early by a re-plan: joins pub
                                         // where the next step (or finish) would have settled it
    bool pending = false;                // the last engine batch's status is still to collect
    bool acc_pending = false;            // acc holds a split step's statuses to settle
    rl_router_stats st{};
};

#define R_OK(x)                                             \
    do {                                                    \
        if ((x) != hipSuccess) return RL_E_DEVICE;          \
    } while (0)
#define R_RC(x)                                             \
    do {                                                    \
        const int _rc = (x);                                \
        if (_rc != RL_OK) return _rc;                       \
    } while (0)

extern "C" void rl_router_destroy(rl_router* r) {
    if (!r) return;
    // the last step's work (on the caller's stream, which may be gone by now: wait on our
    // own event instead)
    if (r->done && r->stepped) (void)hipEventSynchronize(r->done);
    if (r->own) (void)hipStreamSynchronize(r->own);
    void* bufs[] = {r->perm, r->wire_s, r->lim_s, r->hdr2, r->mm_part, r->hdr, r->k_s, r->p_s, r->t_s,
                    r->back_w, r->ret_in, r->dir, r->wire_r, r->lim_r, r->op_r, r->k_r, r->p_r, r->t_r, r->a_r,
                    r->rem_r, r->packed_r, r->ret_out, r->lost, r->acc};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (r->h_hdr) (void)hipHostFree(r->h_hdr);
    if (r->done) (void)hipEventDestroy(r->done);
    if (r->own) (void)hipStreamDestroy(r->own);
    delete r;
}

extern "C" int rl_router_create_ex(rl_engine* e, uint32_t world, uint32_t rank, const rl_transport* t,
                                   const rl_router_opts* opts, rl_router** out) {
    if (!out) return RL_E_INVALID_ARG;
    *out = nullptr;
    if (!e || !t || !t->all_to_all_v || !opts || world == 0 || world > (uint32_t)kMaxShards ||
        (world & (world - 1)) || rank >= world || opts->max_batch == 0 ||
        opts->max_batch > 0xFFFFFFF0ULL)
        return RL_E_INVALID_ARG;
    const size_t n = opts->max_batch;
    size_t m = opts->recv_cap ? opts->recv_cap : std::min<size_t>(world, 2) * n;
    m = std::min(m, engine_max_batch(e));           // the owner's engine decides <= m at once
    if (m == 0) return RL_E_INVALID_ARG;
    rl_router* r = new (std::nothrow) rl_router();
    if (!r) return RL_E_NOMEM;
    r->e = e; r->world = world; r->rank = rank; r->t = *t; r->cap = n; r->rcap = m;
    (void)hipSetDevice(engine_device(e));
    uint64_t bytes = 0;
    auto take = [&](auto** p, size_t b) {
        bytes += b;
        return dev_malloc((void**)p, std::max<size_t>(b, 8)) == hipSuccess;
    };
    r->ret_out_cap = ret_bound(world, m);
    r->ret_in_cap = ret_bound(world, n);
    bool ok = hipStreamCreateWithFlags(&r->own, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&r->done, hipEventDisableTiming) == hipSuccess;
    ok = ok && take(&r->perm, n * 4) && take(&r->wire_s, n * 16) && take(&r->lim_s, n * 2);
    ok = ok && take(&r->k_s, n * 8) && take(&r->p_s, n * 4) && take(&r->t_s, n * 8);
    ok = ok && take(&r->back_w, n * 8) && take(&r->ret_in, r->ret_in_cap);
    ok = ok && take(&r->hdr2, 2 * 8) && take(&r->mm_part, 2 * (size_t)kWireBlocksMax * 8);
    ok = ok && take(&r->hdr, 2 * (size_t)world * kHdrWords * 8) && take(&r->lost, 4);
    ok = ok && take(&r->dir, dir_words(world) * 8);
    ok = ok && take(&r->wire_r, m * 16) && take(&r->lim_r, m * 2) && take(&r->k_r, m * 8);
    ok = ok && take(&r->p_r, m * 4) && take(&r->t_r, m * 8) && take(&r->a_r, m) && take(&r->op_r, m);
    ok = ok && take(&r->rem_r, m * 8) && take(&r->packed_r, m * 8) && take(&r->ret_out, r->ret_out_cap);
    ok = ok && take(&r->acc, kStatusAccWords * 8);
    ok = ok && hipMemset(r->lost, 0, 4) == hipSuccess;
    ok = ok && hipMemset(r->acc, 0, kStatusAccWords * 8) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&r->h_hdr, 2 * (size_t)world * kHdrWords * 8) == hipSuccess;
    if (!ok) { rl_router_destroy(r); return RL_E_NOMEM; }
    r->st.recv_cap = m;
    r->st.reserved_bytes = bytes;
    *out = r;
    return RL_OK;
}

extern "C" int rl_router_create(rl_engine* e, uint32_t world, uint32_t rank, const rl_transport* t,
                                size_t max_batch, rl_router** out) {
    rl_router_opts o{};
    o.max_batch = max_batch;
    return rl_router_create_ex(e, world, rank, t, &o, out);
}

extern "C" int rl_router_stats_get(rl_router* r, rl_router_stats* out) {
    if (!r || !out) return RL_E_INVALID_ARG;
    *out = r->st;
    return RL_OK;
}

// all-to-all with explicit element offsets / counts (host arrays of `world` entries)
static int a2av_at(rl_router* r, const void* send, const uint64_t* so, const uint64_t* sc,
                   void* recv, const uint64_t* ro, const uint64_t* rc, uint64_t bytes, hipStream_t s) {
    const uint32_t G = r->world;
    std::vector<uint64_t> sob(G), scb(G), rob(G), rcb(G);
    for (uint32_t p = 0; p < G; ++p) {
        sob[p] = so[p] * bytes; scb[p] = sc[p] * bytes; rob[p] = ro[p] * bytes; rcb[p] = rc[p] * bytes;
    }
    return r->t.all_to_all_v(r->t.ctx, send, sob.data(), scb.data(), recv, rob.data(), rcb.data(), s) == 0
               ? RL_OK : RL_E_DEVICE;
}

// contiguous segments: offsets are the running sums of the counts
static std::vector<uint64_t> offsets(const std::vector<uint64_t>& c) {
    std::vector<uint64_t> o(c.size());
    uint64_t a = 0;
    for (size_t i = 0; i < c.size(); ++i) { o[i] = a; a += c[i]; }
    return o;
}

static int a2av(rl_router* r, const void* send, const std::vector<uint64_t>& sc, void* recv,
                const std::vector<uint64_t>& rc, uint64_t bytes, hipStream_t s) {
    const std::vector<uint64_t> so = offsets(sc), ro = offsets(rc);
    return a2av_at(r, send, so.data(), sc.data(), recv, ro.data(), rc.data(), bytes, s);
}

// Worse of two statuses (fatal beats invalid-request beats ok; then the lower code).
static int64_t worse(int64_t a, int64_t b) {
    if (a == RL_OK) return b;
    if (b == RL_OK) return a;
    if (fatal(a) != fatal(b)) return fatal(a) ? a : b;
    return std::min(a, b);
}

// The status of this rank's last step's engine batches (the previous step is complete:
// everything before the caller's header exchange or finish). One batch: the engine's own
// collection; a split step: the rounds' statuses folded on device. Either applies the table
// growth the batches asked for, here at the step boundary and never between two rounds.
static int64_t settle_pending(rl_router* r) {
    int64_t st = RL_OK;
    if (r->pending) { st = worse(st, rl_last_status(r->e)); r->pending = false; }
    if (r->acc_pending) {
        unsigned long long h[kStatusAccWords];
        if (r->stepped && hipEventSynchronize(r->done) != hipSuccess) return RL_E_DEVICE;
        if (hipMemcpy(h, r->acc, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemset(r->acc, 0, sizeof(h)) != hipSuccess)
            return RL_E_DEVICE;
        st = worse(st, engine_status_settle(r->e, h));
        r->acc_pending = false;
    }
    return st;
}

// Failure model (include/rl_engine.h: errors are collective). Before the header exchange a
// step may fail on its own (bad arguments, a launch error: nothing has been sent). After
// it, every rank goes through every collective of the step whatever happens locally: all
// buffers exist from creation, an engine call that fails leaves its requests undecided
// (RL_REMAINING_ERROR) and its status is published in the next header, and every rank
// returns it at the same later step (or from rl_router_finish). Every rank derives the
// step's exchange plan (rounds, per-pair ranges) from the same header rows.
//
// Operations (op != NULL) ride in the u16 limiter column (rl_route_fold_ops): the send side has
// no room for a column of their own (the reservation bound of tests/cpp/test_router.cpp), the
// owner decodes the column in place into lim_r and op_r. The column then travels whether or
// not there are limiter ids, so the collectives are those of a step with `limiter`.
extern "C" int rl_router_execute(rl_router* r, size_t n, const uint64_t* key, const int32_t* permits,
                                 const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op,
                                 uint8_t* allowed, int64_t* remaining, void* stream) {
    if (!r) return RL_E_INVALID_ARG;
    if (n > r->cap) return RL_E_TOO_LARGE;          // caller error, before any collective
    if (n && (!key || !permits || !now_ns || !allowed || !remaining)) return RL_E_INVALID_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : r->own;
    const uint32_t G = r->world, me = r->rank;
    rl_engine* e = r->e;
    int64_t* hdr_s = r->hdr;
    int64_t* hdr_r = r->hdr + (size_t)G * kHdrWords;
    // 1. partition (counts into the header on the device) + compact wire records + the
    // batch's now_ms range (per-block partials, folded by the header fill)
    R_RC(rl_route_partition_device(e, n, key, G, r->perm, hdr_s, kHdrWords, s));
    uint32_t nparts = 0;
    const bool col = limiter || op;                  // the u16 column travels
    R_RC(route_pack_wire_mm(e, n, r->perm, key, permits, now_ns, limiter, r->wire_s,
                            limiter && !op ? r->lim_s : nullptr, r->hdr2, r->mm_part, &nparts, s));
    if (op) R_RC(rl_route_fold_ops(e, n, r->perm, limiter, op, r->lim_s, s));
    R_OK(launch_fill_header(hdr_s, r->hdr2, r->pub, (int64_t)r->cap, (int64_t)r->rcap, G, r->mm_part,
                            nparts, s));
    // 2. header exchange and the step's one host synchronisation
    const std::vector<uint64_t> hw(G, kHdrWords);
    R_RC(a2av(r, hdr_s, hw, hdr_r, hw, 8, s));
    R_OK(hipMemcpyAsync(r->h_hdr, r->hdr, 2 * (size_t)G * kHdrWords * 8, hipMemcpyDeviceToHost, s));
    const auto c0 = std::chrono::steady_clock::now();
    R_OK(hipStreamSynchronize(s));
    const auto c1 = std::chrono::steady_clock::now();
    r->st.header_sync_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(c1 - c0).count();
    ++r->st.steps;
    // count matrix C[src][owner] from every source's row (the same on every rank)
    std::vector<uint64_t> C((size_t)G * G);
    std::vector<int64_t> base(G);
    bool wide = false, cap_mismatch = false;
    int64_t worst = RL_OK, tmin = INT64_MAX, tmax = INT64_MIN;
    for (uint32_t p = 0; p < G; ++p) {
        const int64_t* rcv = r->h_hdr + (size_t)(G + p) * kHdrWords;
        for (uint32_t o = 0; o < G; ++o) C[(size_t)p * G + o] = (uint64_t)rcv[kHdrFixed + o];
        base[p] = rcv[1];
        wide |= rcv[2] != 0;
        if (fatal(rcv[3])) worst = worse(worst, rcv[3]);
        cap_mismatch |= rcv[4] != (int64_t)r->cap || rcv[7] != (int64_t)r->rcap;
        if (rcv[0]) { tmin = std::min(tmin, rcv[5]); tmax = std::max(tmax, rcv[6]); }
    }
    // the previous batch is complete (ordered before the header exchange): its status is
    // published in the next header; the statuses received now (every rank's batch two steps
    // back) are the same on all ranks, so all fail together
    if (fatal(r->pub)) r->pub = RL_OK;              // delivered: every rank returns it now, once
    r->pub = worse(r->pub, worse(r->held, settle_pending(r)));
    r->held = RL_OK;
    // every rank sees every rank's capacities: a mismatch fails all of them here, before
    // any payload (all ranks must derive the same exchange plan)
    if (worst != RL_OK || cap_mismatch) {
        // this step's own requests are not decided: say so in its outputs, so that a caller
        // that goes on does not read the previous step's decisions as this one's
        R_OK(launch_fill_value(allowed, remaining, (uint32_t)n, RL_REMAINING_ERROR, s));
        R_OK(hipEventRecord(r->done, s));
        r->stepped = true;
        return worst != RL_OK ? (int)worst : RL_E_INVALID_ARG;
    }
    // rounds: each owner's incoming stream (sources in rank order = global arrival order)
    // is cut into pieces of at most rcap requests; round k moves piece k of every owner
    // (rl_exchange.hpp)
    const ExchangePlan plan = exchange_plan(C, G, me, r->rcap);
    const std::vector<uint64_t>& counts = plan.counts;   // mine to each owner
    const std::vector<uint64_t>& rc = plan.rc;           // each source's to me
    const uint64_t rounds = plan.rounds, m = plan.m;
    r->st.max_recv = std::max<uint64_t>(r->st.max_recv, m);
    r->st.rounds += rounds;
    int64_t local = RL_OK;                           // this step's own failure, published later
    const bool far = m && tmax > tmin && (uint64_t)(tmax - tmin) >= ((uint64_t)1 << 31) - 1;
    if (!wide && rounds == 1) {
        // 3. payload: 16-B wire records (+ limiter ids)
        R_RC(a2av(r, r->wire_s, counts, r->wire_r, rc, 16, s));
        if (col) R_RC(a2av(r, r->lim_s, counts, r->lim_r, rc, 2, s));
        if (op) R_RC(rl_route_unfold_ops(e, m, r->lim_r, r->lim_r, r->op_r, s));
        R_RC(rl_route_unwire(e, m, r->wire_r, G, base.data(), rc.data(), r->k_r, r->p_r, r->t_r, s));
        // 4. the owner decides. The merged batch spans the sources' real time range; past
        // what the engine's compact records hold (+-2^31 ms around its first request) it runs
        // in full-width records (skewed clocks across front-ends).
        if (far) (void)rl_tune(e, "wide_records", 1);
        const int xrc = engine_execute_routed(e, m, r->k_r, r->p_r, r->t_r, col ? r->lim_r : nullptr,
                                                op ? r->op_r : nullptr, r->a_r, r->rem_r, nullptr, s);
        if (far) (void)rl_tune(e, "wide_records", 0);
        if (xrc != RL_OK) {
            local = xrc;
            R_OK(launch_fill_value(r->a_r, r->rem_r, (uint32_t)m, RL_REMAINING_ERROR, s));
        } else {
            r->pending = true;
        }
        // 5. decisions back, segmented with exception blocks
        int W = rl_result_width(e);
        if (W < 0) { local = worse(local, W); W = 8; }
        R_RC(rl_route_fold_return(e, m, r->a_r, r->rem_r, r->ret_out, W, G, rc.data(), kExcCap, s));
        std::vector<uint64_t> seg_o(G), seg_i(G);
        for (uint32_t p = 0; p < G; ++p) {
            seg_o[p] = rl_route_return_bytes(1, &rc[p], W, kExcCap);
            seg_i[p] = rl_route_return_bytes(1, &counts[p], W, kExcCap);
        }
        R_RC(a2av(r, r->ret_out, seg_o, r->ret_in, seg_i, 1, s));
        // 6. back to the caller's order
        R_RC(rl_route_unpack_return(e, n, r->perm, r->ret_in, W, G, counts.data(), kExcCap, allowed,
                                    remaining, r->lost, s));
    } else {
        // Wide layout (a source's batch spans more than 2^31 ms: SoA payload) and/or several
        // rounds (some owner receives more than rcap requests): 8-B decisions back into
        // back_w at each request's owner-order position, one unpack at the end.
        // (the column is already in lim_s: the wire pack or the ops fold wrote it)
        if (wide) R_RC(rl_route_pack(e, n, r->perm, key, permits, now_ns, limiter, r->k_s, r->p_s,
                                     r->t_s, nullptr, s));
        if (rounds > 1) ++r->st.split_steps;
        for (uint64_t k = 0; k < rounds; ++k) {
            const ExchangeRound X = exchange_round(plan, k);
            const std::vector<uint64_t>&so = X.so, &sc = X.sc, &ro = X.ro, &rr = X.rr;
            const uint64_t mk = X.mk;
            if (!wide) {
                R_RC(a2av_at(r, r->wire_s, so.data(), sc.data(), r->wire_r, ro.data(), rr.data(), 16, s));
                if (col)
                    R_RC(a2av_at(r, r->lim_s, so.data(), sc.data(), r->lim_r, ro.data(), rr.data(), 2, s));
                R_RC(rl_route_unwire(e, mk, r->wire_r, G, base.data(), rr.data(), r->k_r, r->p_r, r->t_r, s));
            } else {
                R_RC(a2av_at(r, r->k_s, so.data(), sc.data(), r->k_r, ro.data(), rr.data(), 8, s));
                R_RC(a2av_at(r, r->p_s, so.data(), sc.data(), r->p_r, ro.data(), rr.data(), 4, s));
                R_RC(a2av_at(r, r->t_s, so.data(), sc.data(), r->t_r, ro.data(), rr.data(), 8, s));
                if (col)
                    R_RC(a2av_at(r, r->lim_s, so.data(), sc.data(), r->lim_r, ro.data(), rr.data(), 2, s));
            }
            if (op) R_RC(rl_route_unfold_ops(e, mk, r->lim_r, r->lim_r, r->op_r, s));
            const bool w = wide || far;
            if (w) (void)rl_tune(e, "wide_records", 1);
            const int xrc = engine_execute_routed(e, mk, r->k_r, r->p_r, r->t_r,
                                                    col ? r->lim_r : nullptr, op ? r->op_r : nullptr,
                                                    r->a_r, r->rem_r, nullptr, s);
            if (w) (void)rl_tune(e, "wide_records", 0);
            if (xrc != RL_OK) {
                local = worse(local, xrc);
                R_OK(launch_fill_value(r->a_r, r->rem_r, (uint32_t)mk, RL_REMAINING_ERROR, s));
            } else {
                // the round's data-dependent status is folded on device (the next round's
                // batch replaces the engine's own) and settled at the next step: no host
                // synchronisation and no table growth between the rounds' collectives
                R_RC(engine_status_accum(e, r->acc, s));
                r->acc_pending = true;
            }
            R_RC(rl_route_fold(e, mk, r->a_r, r->rem_r, r->packed_r, s));
            R_RC(a2av_at(r, r->packed_r, ro.data(), rr.data(), r->back_w, so.data(), sc.data(), 8, s));
        }
        R_RC(rl_route_unpack(e, n, r->perm, r->back_w, allowed, remaining, s));
    }
    if (local != RL_OK) r->pub = worse(r->pub, local);   // published in the next header
    R_OK(hipEventRecord(r->done, s));
    r->stepped = true;
    return RL_OK;
}

extern "C" int rl_router_step(rl_router* r, size_t n, const uint64_t* key, const int32_t* permits,
                              const int64_t* now_ns, const uint16_t* limiter, uint8_t* allowed,
                              int64_t* remaining, void* stream) {
    return rl_router_execute(r, n, key, permits, now_ns, limiter, nullptr, allowed, remaining, stream);
}

extern "C" int rl_router_finish(rl_router* r) {
    if (!r) return RL_E_INVALID_ARG;
    hipStream_t s = r->own;
    // the last step may still run on the caller's stream (its return all-to-all and the
    // unpack that counts lost remainders): complete it before reading anything
    if (r->stepped) R_OK(hipEventSynchronize(r->done));
    r->pub = worse(r->pub, worse(r->held, settle_pending(r)));
    r->held = RL_OK;
    uint32_t lost = 0;
    R_OK(hipMemcpy(&lost, r->lost, 4, hipMemcpyDeviceToHost));
    if (lost) R_OK(hipMemset(r->lost, 0, 4));        // counted once: the next steps start clean
    const int64_t mine = lost ? worse(r->pub, (int64_t)RL_E_CAPACITY) : r->pub;
    r->pub = RL_OK;                                  // reported now, on every rank
    const uint32_t G = r->world;
    int64_t* hdr_s = r->hdr;
    int64_t* hdr_r = r->hdr + (size_t)G;
    std::vector<int64_t> row(G, mine);
    R_OK(hipMemcpyAsync(hdr_s, row.data(), G * 8, hipMemcpyHostToDevice, s));
    const std::vector<uint64_t> one(G, 1);
    R_RC(a2av(r, hdr_s, one, hdr_r, one, 8, s));
    std::vector<int64_t> got(G);
    R_OK(hipMemcpyAsync(got.data(), hdr_r, G * 8, hipMemcpyDeviceToHost, s));
    R_OK(hipStreamSynchronize(s));
    int64_t w = RL_OK;
    for (int64_t x : got) w = worse(w, x);
    return (int)w;
}

// The directory plan (DirPlan, rl_replan.hpp) shared by rl_router_plan_directory and
// rl_router_replan_directory (collective): every rank's candidates merged, the k hottest kept
// and placed on owners by longest-processing-time-first. Every rank computes the same plan;
// nothing is installed.
static int plan_directory(rl_router* r, size_t n, const uint64_t* key, const uint64_t* count,
                          uint64_t sampled, uint32_t k, hipStream_t s, DirPlan* plan) {
    const uint32_t G = r->world;
    // exchange {n, sampled}, then every rank's candidates with every rank (all-gather), in
    // the buffer reserved at creation (no allocation between the two collectives)
    uint64_t* d = r->dir;                          // [2G] sent rows, [2G] received rows
    uint64_t* ds = d + 4 * (size_t)G;              // [2 kDirMax] my candidates
    uint64_t* dr = ds + 2 * (size_t)kDirMax;       // [2 kDirMax G] everyone's
    std::vector<uint64_t> mine(2 * (size_t)G);
    for (uint32_t p = 0; p < G; ++p) { mine[2 * p] = n; mine[2 * p + 1] = sampled; }
    const std::vector<uint64_t> two(G, 2);
    std::vector<uint64_t> peer(2 * (size_t)G);
    R_OK(hipMemcpyAsync(d, mine.data(), G * 16, hipMemcpyHostToDevice, s));
    R_RC(a2av(r, d, two, d + 2 * G, two, 8, s));
    R_OK(hipMemcpyAsync(peer.data(), d + 2 * G, G * 16, hipMemcpyDeviceToHost, s));
    R_OK(hipStreamSynchronize(s));
    uint64_t total_n = 0, total_sampled = 0;
    std::vector<uint64_t> rb(G), sb(G, 2 * (uint64_t)n), so(G, 0), ro(G);
    for (uint32_t p = 0; p < G; ++p) {
        rb[p] = 2 * peer[2 * p];
        total_n += peer[2 * p];
        total_sampled += peer[2 * p + 1];
    }
    uint64_t acc = 0;
    for (uint32_t p = 0; p < G; ++p) { ro[p] = acc; acc += rb[p]; }
    std::vector<uint64_t> cand(2 * std::max<size_t>(n, 1)), all(2 * std::max<uint64_t>(total_n, 1));
    for (size_t i = 0; i < n; ++i) { cand[2 * i] = key[i]; cand[2 * i + 1] = count[i]; }
    R_OK(hipMemcpyAsync(ds, cand.data(), n * 16, hipMemcpyHostToDevice, s));
    // every peer gets the same block: send offsets all 0
    R_RC(a2av_at(r, ds, so.data(), sb.data(), dr, ro.data(), rb.data(), 8, s));
    R_OK(hipMemcpyAsync(all.data(), dr, total_n * 16, hipMemcpyDeviceToHost, s));
    R_OK(hipStreamSynchronize(s));
    // merge (same order on every rank), keep the k hottest, place them LPT-first
    std::map<uint64_t, uint64_t> sum;
    for (uint64_t i = 0; i < total_n; ++i) sum[all[2 * i]] += all[2 * i + 1];
    std::vector<std::pair<uint64_t, uint64_t>> v(sum.begin(), sum.end());
    std::sort(v.begin(), v.end(), [](const auto& a, const auto& b) {
        return a.second != b.second ? a.second > b.second : a.first < b.first;
    });
    if (v.size() > k) v.resize(k);
    uint64_t hot = 0;
    for (auto& x : v) hot += x.second;
    const double rest = total_sampled > hot ? (double)(total_sampled - hot) / G : 0.0;
    std::vector<double> load(G, rest);
    plan->key.resize(v.size());
    plan->owner.resize(v.size());
    for (size_t i = 0; i < v.size(); ++i) {
        uint32_t best = 0;
        for (uint32_t p = 1; p < G; ++p)
            if (load[p] < load[best]) best = p;
        load[best] += (double)v[i].second;
        plan->key[i] = v[i].first;
        plan->owner[i] = best;
    }
    return RL_OK;
}

extern "C" int rl_router_plan_directory(rl_router* r, size_t n, const uint64_t* key,
                                        const uint64_t* count, uint64_t sampled, uint32_t k,
                                        uint32_t* placed, void* stream) {
    if (!r || (n && (!key || !count)) || n > kDirMax || k > kDirMax) return RL_E_INVALID_ARG;
    DirPlan plan;
    R_RC(plan_directory(r, n, key, count, sampled, k, stream ? (hipStream_t)stream : r->own, &plan));
    const int rc = rl_set_owner_directory(r->e, plan.key.size(), plan.key.data(), plan.owner.data());
    if (rc == RL_OK && placed) *placed = (uint32_t)plan.key.size();
    return rc;
}

// This rank's top keys of a device sample, on the host (the candidates of the two _sampled
// calls). A failure of this rank alone must not leave the others waiting in the collective
// that follows: the caller goes on with no candidates and reports the status afterwards.
static int sample_candidates(rl_router* r, size_t n, const uint64_t* key_hash, uint32_t k,
                             uint64_t min_count, hipStream_t s, std::vector<uint64_t>* key,
                             std::vector<uint64_t>* cnt) {
    // the candidates land in the exchange buffer, which the plan rewrites only after they are
    // on the host: keys and counts where it puts its candidates ([2 kDirMax]), the header at
    // the start of the receive area
    uint64_t* dk = r->dir + 4 * (size_t)r->world;
    uint64_t* dc = dk + kDirMax;
    uint64_t* dh = dc + kDirMax;
    uint64_t hdr[4] = {0, 0, 0, 0};
    int mine = rl_top_keys_device(r->e, n, key_hash, k, min_count, dk, dc, dh, s);
    if (mine == RL_OK) {
        if (hipMemcpyAsync(hdr, dh, sizeof(hdr), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            mine = RL_E_DEVICE;
        else if (hdr[2])
            mine = RL_E_CAPACITY;
        else if (hdr[0] > kDirMax)
            mine = RL_E_INTERNAL;
    }
    if (mine == RL_OK && hdr[0]) {
        key->resize(hdr[0]);
        cnt->resize(hdr[0]);
        if (hipMemcpy(key->data(), dk, hdr[0] * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(cnt->data(), dc, hdr[0] * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            mine = RL_E_DEVICE;
            key->clear();
            cnt->clear();
        }
    }
    return mine;
}

extern "C" int rl_router_plan_directory_sampled(rl_router* r, size_t n, const uint64_t* key_hash,
                                                uint32_t k, uint64_t min_count, uint32_t* placed,
                                                void* stream) {
    // argument errors, as rl_router_plan_directory's, return before the collective (every
    // rank passes the same k and min_count)
    if (!r || (n && !key_hash) || k == 0 || k > kDirMax || min_count == 0 || (uint64_t)n > (1ULL << 31))
        return RL_E_INVALID_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : r->own;
    std::vector<uint64_t> key, cnt;
    const int mine = sample_candidates(r, n, key_hash, k, min_count, s, &key, &cnt);
    const int rc = rl_router_plan_directory(r, key.size(), key.data(), cnt.data(), (uint64_t)n, k,
                                            placed, s);
    return mine != RL_OK ? mine : rc;
}

// ---------------------------------------------------------------- re-plan on a live router
// (which keys move, and the images grouped by new owner: rl_replan.hpp)
namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};
}  // namespace

// One row of `words` u64 from every rank to every rank (through the exchange buffer's header
// rows: words <= 2); got[p * words + w] = rank p's word w.
static int gather_rows(rl_router* r, const uint64_t* mine, uint32_t words, std::vector<uint64_t>* got,
                       hipStream_t s) {
    const uint32_t G = r->world;
    uint64_t* d = r->dir;
    got->assign((size_t)G * words, 0);
    const std::vector<uint64_t> sb(G, words), so(G, 0);
    const std::vector<uint64_t> ro = offsets(sb);
    R_OK(hipMemcpyAsync(d, mine, words * 8, hipMemcpyHostToDevice, s));
    R_RC(a2av_at(r, d, so.data(), sb.data(), d + 2 * G, ro.data(), sb.data(), 8, s));
    R_OK(hipMemcpyAsync(got->data(), d + 2 * G, (size_t)G * words * 8, hipMemcpyDeviceToHost, s));
    R_OK(hipStreamSynchronize(s));
    return RL_OK;
}

// `mine0`: a status of this rank from before the collective (its sample failed: it took part
// with no candidates), returned after a re-plan that otherwise succeeded.
static int replan(rl_router* r, size_t n, const uint64_t* key, const uint64_t* count, uint64_t sampled,
                  uint32_t k, uint32_t* placed, uint64_t* moved, int mine0, hipStream_t s) {
    const uint32_t G = r->world, me = r->rank;
    rl_engine* e = r->e;
    // 1. drain: this rank's previous step is complete, and its engine status is settled (the
    // table growth it asked for applied) as the next step would have done; that step, or
    // rl_router_finish, still publishes it, so it is reported when it would have been
    if (r->stepped) R_OK(hipEventSynchronize(r->done));
    r->held = worse(r->held, settle_pending(r));
    // 2. plan D' and the movers from D to D' (the same on every rank)
    DirPlan d_new, d_old;
    R_RC(plan_directory(r, n, key, count, sampled, k, s, &d_new));
    d_old.key.resize(kDirMax);
    d_old.owner.resize(kDirMax);
    const size_t n_old = engine_directory(e, d_old.key.data(), d_old.owner.data());
    d_old.key.resize(n_old);
    d_old.owner.resize(n_old);
    const std::vector<Mover> M = mover_list(d_old, d_new, [&](uint64_t key) { return rl_owner_of(key, 0, G); });
    const std::vector<uint64_t> mine_keys = movers_from(M, me);   // the movers this rank owns under D
    // 3. copy my movers' images, grouped by new owner; counts, buffers, then a status row
    int64_t local = RL_OK;
    std::vector<rl_key_image> imgs(mine_keys.size() * std::max<size_t>(engine_limiters(e), 1));
    size_t n_img = 0;
    local = rl_copy_keys(e, mine_keys.size(), mine_keys.data(), imgs.data(), imgs.size(), &n_img);
    if (local != RL_OK) n_img = 0;
    imgs.resize(n_img);
    const std::vector<uint64_t> sc = group_by_new_owner(&imgs, M, G);
    std::vector<uint64_t> rc(G, 0);
    {
        const std::vector<uint64_t> one(G, 1);
        uint64_t* d = r->dir;
        R_OK(hipMemcpyAsync(d, sc.data(), G * 8, hipMemcpyHostToDevice, s));
        R_RC(a2av(r, d, one, d + 2 * G, one, 8, s));
        R_OK(hipMemcpyAsync(rc.data(), d + 2 * G, G * 8, hipMemcpyDeviceToHost, s));
        R_OK(hipStreamSynchronize(s));
    }
    uint64_t n_recv = 0;
    for (uint32_t p = 0; p < G; ++p) n_recv += rc[p];
    DevBuf b_send, b_recv;                           // (freed on every way out)
    (void)hipSetDevice(engine_device(e));
    if (dev_malloc(&b_send.p, std::max<size_t>(n_img, 1) * sizeof(rl_key_image)) != hipSuccess ||
        dev_malloc(&b_recv.p, std::max<size_t>(n_recv, 1) * sizeof(rl_key_image)) != hipSuccess)
        local = worse(local, RL_E_NOMEM);
    rl_key_image* d_send = (rl_key_image*)b_send.p;
    rl_key_image* d_recv = (rl_key_image*)b_recv.p;
    std::vector<uint64_t> row;
    const uint64_t st1[2] = {(uint64_t)local, (uint64_t)n_img};
    R_RC(gather_rows(r, st1, 2, &row, s));
    int64_t worst = RL_OK;
    uint64_t total = 0;
    for (uint32_t p = 0; p < G; ++p) { worst = worse(worst, (int64_t)row[2 * p]); total += row[2 * p + 1]; }
    if (worst != RL_OK) return (int)worst;           // nothing has changed; D stays installed
    // 4. move: the images to their new owners, which put them; a second status row
    std::vector<rl_key_image> got(n_recv);
    if (n_img) R_OK(hipMemcpyAsync(d_send, imgs.data(), n_img * sizeof(rl_key_image), hipMemcpyHostToDevice, s));
    R_RC(a2av(r, d_send, sc, d_recv, rc, sizeof(rl_key_image), s));
    if (n_recv) R_OK(hipMemcpyAsync(got.data(), d_recv, n_recv * sizeof(rl_key_image), hipMemcpyDeviceToHost, s));
    R_OK(hipStreamSynchronize(s));
    local = rl_put_keys(e, got.size(), got.data(), nullptr);
    const uint64_t st2[1] = {(uint64_t)local};
    R_RC(gather_rows(r, st2, 1, &row, s));
    for (uint32_t p = 0; p < G; ++p) worst = worse(worst, (int64_t)row[p]);
    // 5. commit (the old owners drop their movers, every rank installs D'), or roll back (the
    // new owners drop what they put: they held no state for those keys under D; D stays)
    if (worst != RL_OK) {
        std::vector<uint64_t> back(got.size());
        for (size_t i = 0; i < got.size(); ++i) back[i] = got[i].key_hash;
        std::sort(back.begin(), back.end());
        back.erase(std::unique(back.begin(), back.end()), back.end());
        const int drc = rl_drop_keys(e, back.size(), back.data(), nullptr);
        return drc != RL_OK && !fatal(worst) ? drc : (int)worst;
    }
    R_RC(rl_drop_keys(e, mine_keys.size(), mine_keys.data(), nullptr));
    R_RC(rl_set_owner_directory(e, d_new.key.size(), d_new.key.data(), d_new.owner.data()));
    if (placed) *placed = (uint32_t)d_new.key.size();
    if (moved) *moved = total;
    return mine0;
}

extern "C" int rl_router_replan_directory(rl_router* r, size_t n, const uint64_t* key,
                                          const uint64_t* count, uint64_t sampled, uint32_t k,
                                          uint32_t* placed, uint64_t* moved, void* stream) {
    if (!r || (n && (!key || !count)) || n > kDirMax || k > kDirMax) return RL_E_INVALID_ARG;
    return replan(r, n, key, count, sampled, k, placed, moved, RL_OK, stream ? (hipStream_t)stream : r->own);
}

extern "C" int rl_router_replan_directory_sampled(rl_router* r, size_t n, const uint64_t* key_hash,
                                                  uint32_t k, uint64_t min_count, uint32_t* placed,
                                                  uint64_t* moved, void* stream) {
    if (!r || (n && !key_hash) || k == 0 || k > kDirMax || min_count == 0 || (uint64_t)n > (1ULL << 31))
        return RL_E_INVALID_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : r->own;
    // the sample reads no limiter state, but it runs on the engine behind the previous step
    std::vector<uint64_t> key, cnt;
    const int mine = sample_candidates(r, n, key_hash, k, min_count, s, &key, &cnt);
    return replan(r, key.size(), key.data(), cnt.data(), (uint64_t)n, k, placed, moved, mine, s);
}

// ---------------------------------------------------------------- retry-after, collectively
// The step's exchange with three differences: only the queries with skip == 0 are placed
// (rl_route_partition_skip_device; the wire pack takes their count from the header column on
// the device, where the partition left it, since the host learns it only from the header
// read), the owner answers with rl_retry_after_device into rem_r, and the waits come back
// 8 B each into back_w at the query's owner-order position, whatever the number of rounds.
// It reads and writes none of pub / held / pending / acc and none of the step statistics; its
// header row carries status 0 and the received statuses are not looked at.
//
// Failure model: argument errors and launch errors before the header exchange return at once
// (nothing has been sent). After it every rank goes through every collective: a local failure
// is kept in `local`, an owner that could not answer sends RL_RETRY_ERROR, and one status row
// (gather_rows, as the re-plan's) makes every rank return the worst status.
extern "C" int rl_router_retry_after(rl_router* r, size_t n, const uint64_t* key, const int32_t* permits,
                                     const int64_t* now_ns, const uint16_t* limiter,
                                     const uint8_t* skip, int64_t* wait_ms, void* stream) {
    if (!r) return RL_E_INVALID_ARG;
    if (n > r->cap) return RL_E_TOO_LARGE;          // caller error, before any collective
    if (n && (!key || !permits || !now_ns || !wait_ms)) return RL_E_INVALID_ARG;
    hipStream_t s = stream ? (hipStream_t)stream : r->own;
    const uint32_t G = r->world, me = r->rank;
    rl_engine* e = r->e;
    int64_t* hdr_s = r->hdr;
    int64_t* hdr_r = r->hdr + (size_t)G * kHdrWords;
    // behind this rank's previous step: its queued work still uses the exchange buffers
    if (r->stepped) R_OK(hipStreamWaitEvent(s, r->done, 0));
    R_RC(rl_route_partition_skip_device(e, n, key, skip, G, r->perm, hdr_s, kHdrWords, s));
    uint32_t nparts = 0;
    R_RC(route_pack_wire_mm(e, n, r->perm, key, permits, now_ns, limiter, r->wire_s,
                            limiter ? r->lim_s : nullptr, r->hdr2, r->mm_part, &nparts, s, hdr_s,
                            kHdrWords, G));
    R_OK(launch_fill_header(hdr_s, r->hdr2, RL_OK, (int64_t)r->cap, (int64_t)r->rcap, G, r->mm_part,
                            nparts, s));
    const std::vector<uint64_t> hw(G, kHdrWords);
    R_RC(a2av(r, hdr_s, hw, hdr_r, hw, 8, s));
    R_OK(hipMemcpyAsync(r->h_hdr, r->hdr, 2 * (size_t)G * kHdrWords * 8, hipMemcpyDeviceToHost, s));
    R_OK(hipStreamSynchronize(s));
    std::vector<uint64_t> C((size_t)G * G);
    std::vector<int64_t> base(G);
    bool wide = false, cap_mismatch = false;
    for (uint32_t p = 0; p < G; ++p) {
        const int64_t* rcv = r->h_hdr + (size_t)(G + p) * kHdrWords;
        for (uint32_t o = 0; o < G; ++o) C[(size_t)p * G + o] = (uint64_t)rcv[kHdrFixed + o];
        base[p] = rcv[1];
        wide |= rcv[2] != 0;
        cap_mismatch |= rcv[4] != (int64_t)r->cap || rcv[7] != (int64_t)r->rcap;
    }
    if (cap_mismatch) {                              // seen by every rank: all return here
        R_OK(launch_fill_i64(wait_ms, (uint32_t)n, RL_RETRY_ERROR, s));
        R_OK(hipStreamSynchronize(s));
        return RL_E_INVALID_ARG;
    }
    const ExchangePlan plan = exchange_plan(C, G, me, r->rcap);
    uint64_t n_live = 0;
    for (uint32_t o = 0; o < G; ++o) n_live += plan.counts[o];
    int64_t local = RL_OK;
    auto keep = [&](int rc) { if (rc != RL_OK) local = worse(local, rc); return rc; };
    auto hip = [&](hipError_t x) { return x == hipSuccess ? RL_OK : RL_E_DEVICE; };
    if (wide) keep(rl_route_pack(e, n_live, r->perm, key, permits, now_ns, limiter, r->k_s, r->p_s,
                                 r->t_s, nullptr, s));
    for (uint64_t k = 0; k < plan.rounds; ++k) {
        const ExchangeRound X = exchange_round(plan, k);
        const uint64_t *so = X.so.data(), *sc = X.sc.data(), *ro = X.ro.data(), *rr = X.rr.data();
        int orc = RL_OK;                             // can this owner answer the round?
        if (!wide) {
            orc = worse(orc, keep(a2av_at(r, r->wire_s, so, sc, r->wire_r, ro, rr, 16, s)));
            if (limiter) orc = worse(orc, keep(a2av_at(r, r->lim_s, so, sc, r->lim_r, ro, rr, 2, s)));
            if (orc == RL_OK)
                orc = keep(rl_route_unwire(e, X.mk, r->wire_r, G, base.data(), rr, r->k_r, r->p_r, r->t_r, s));
        } else {
            orc = worse(orc, keep(a2av_at(r, r->k_s, so, sc, r->k_r, ro, rr, 8, s)));
            orc = worse(orc, keep(a2av_at(r, r->p_s, so, sc, r->p_r, ro, rr, 4, s)));
            orc = worse(orc, keep(a2av_at(r, r->t_s, so, sc, r->t_r, ro, rr, 8, s)));
            if (limiter) orc = worse(orc, keep(a2av_at(r, r->lim_s, so, sc, r->lim_r, ro, rr, 2, s)));
        }
        if (orc == RL_OK)
            orc = keep(rl_retry_after_device(e, X.mk, r->k_r, r->p_r, r->t_r, limiter ? r->lim_r : nullptr,
                                             nullptr, r->rem_r, s));
        if (orc != RL_OK) keep(hip(launch_fill_i64(r->rem_r, (uint32_t)X.mk, RL_RETRY_ERROR, s)));
        keep(a2av_at(r, r->rem_r, ro, rr, r->back_w, so, sc, 8, s));
    }
    keep(rl_route_unpack_wait(e, n, n_live, r->perm, r->back_w, skip, wait_ms, s));
    // one status row, then the synchronous end (gather_rows synchronises the stream)
    std::vector<uint64_t> row;
    const uint64_t mine[1] = {(uint64_t)local};
    R_RC(gather_rows(r, mine, 1, &row, s));
    int64_t worst = RL_OK;
    for (uint32_t p = 0; p < G; ++p) worst = worse(worst, (int64_t)row[p]);
    return (int)worst;
}
