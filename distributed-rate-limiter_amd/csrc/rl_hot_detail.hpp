// rl_hot_detail.hpp — the hot chains' per-chain and per-key state (Chain, ChainDbg, KeyChain)
// and the record-by-record path of one chunk (detail). Included by rl_hot.hpp.
#pragma once
#include "rl_hot_thresh.hpp"
#include "rl_hot_words.hpp"

#pragma clang fp contract(off)

// The chain's parts are functions for the reader only: each is inlined into its caller (a call
// would spill the chain's registers around it).
#define RL_PART __device__ __attribute__((always_inline)) inline

namespace rl {

// A chain's debug counters and cycle stamps (RegionArgs::dbg; kDbgWords words per region).
struct ChainDbg {
    bool on = false;
    uint64_t t_start = 0;
    uint32_t n_detail = 0, n_other = 0;               // detailed chunks, other keys' records
    uint32_t n_changed = 0, n_tk = 0, n_fb = 0;       // state changes, [T0, T1) updates,
    uint32_t n_late = 0;                              // detailed chunks starting before T0 / ending past T1
    uint32_t n_prehit = 0;                            // chunks whose records were prefetched
    uint32_t n_bisect = 0;                            // SW table entries found by bisection (per lane)
    uint32_t n_sw_it = 0;                             // SW greedy steps
    uint32_t n_walk = 0, n_find = 0, n_enter = 0;     // walked allows, table steps, block loads
    uint64_t cyc_build = 0;                           // SW table builds
    uint64_t cyc_run = 0, cyc_search = 0, cyc_detail = 0, cyc_pre = 0;
    uint64_t cyc_pass1 = 0, cyc_pass2 = 0;
    uint64_t cyc_sw[4] = {0, 0, 0, 0};                // SW run: setup, greedy, remaining, commit
    uint64_t cyc_find = 0, cyc_walk = 0;              // walk cycles (finding / all)
    uint64_t cyc_close = 0, cyc_allow = 0;            // walk cycles (verdicts / allows)

    // a measured section: `c = now(); ...; add(acc, c)`, or `c2 = lap(acc, c)` where the next
    // section starts at the same stamp
    RL_PART uint64_t now() const { return on ? __builtin_amdgcn_s_memtime() : 0; }
    RL_PART void add(uint64_t& acc, uint64_t since) const {
        if (on) acc += __builtin_amdgcn_s_memtime() - since;
    }
    RL_PART uint64_t lap(uint64_t& acc, uint64_t since) const {
        const uint64_t c = now();
        if (on) acc += c - since;
        return c;
    }
    // top bit of d[3]: a hot region; its bits 0-31: detailed chunks, 32-47 / 48-62: threshold
    // updates / chunks starting before T0 (saturating); d[7]: changes | late chunks << 24
    // (saturating)
    RL_PART void store(uint64_t* d, uint32_t records) const {
        d[0] = t_start; d[1] = __builtin_amdgcn_s_memrealtime(); d[2] = records;
        d[3] = (uint64_t)n_detail | (uint64_t)min(n_tk, 0xFFFFu) << 32 | (uint64_t)min(n_fb, 0x7FFFu) << 48 | (1ULL << 63);
        d[4] = cyc_detail; d[5] = cyc_run; d[6] = cyc_search;
        d[7] = min((uint64_t)n_changed, (uint64_t)0xFFFFFF) | min((uint64_t)n_late, (uint64_t)0xFFFFFF) << 24;
        d[8] = cyc_pre; d[9] = cyc_pass1; d[10] = cyc_pass2; d[11] = n_other; d[12] = n_prehit;
        d[13] = cyc_build; d[14] = n_bisect;
        d[15] = cyc_sw[0]; d[16] = cyc_sw[1]; d[17] = cyc_sw[2]; d[18] = cyc_sw[3]; d[19] = n_sw_it;
        d[20] = n_walk; d[21] = n_find; d[22] = cyc_find; d[23] = cyc_walk;
        d[24] = cyc_close; d[25] = cyc_allow; d[26] = n_enter;
    }
};

// What every part of one chain reads of its region (wave-uniform, constant once the region is
// loaded), and the chain's results.
template <class Codec, class Res_, bool TOK_>
struct Chain {
    using CodecT = Codec;
    using Rec = typename Codec::Rec;
    using Res = Res_;
    static constexpr bool TOK = TOK_;
    const RegionArgs& a;
    RegionLds<Codec, true>& S;
    const HotInfo& f;
    const DevLimiter& L;
    const uint32_t i, lane;
    const int64_t base, lo, hi;                       // the batch's time base and range
    const Rec* recs;
    // the keys' slots in the LDS image. hot_ok false (no dominant key, or its region is full):
    // pass 2 takes every record; the second key has a chain only beside the first's
    int32_t hsl0 = -1, hsl1 = -1;
    bool hot_ok = false, hot_ok2 = false;
    uint32_t n_allowed = 0, n_invalid = 0, n_caperr = 0, n_rounds = 0;
    uint32_t n_internal = 0;                          // walk logic errors (RL_E_INTERNAL, uniform)
    bool any_hot = false;
    ChainDbg dbg;

    RL_PART bool is_hot(const Req& q, bool valid) const {
        return valid && !q.invalid && ((hot_ok && q.h == f.tag) || (hot_ok2 && q.h == f.tag2));
    }
    // summary words of chunk c / group g
    RL_PART uint64_t* summ_at(uint32_t c) const {
        return a.hot_summ + (size_t)(f.chunk_base + (c < f.n_chunks ? c : 0)) * hotw::kEntryWords;
    }
    RL_PART uint64_t* grp_at(uint32_t g) const {
        return a.hot_summ2 + (size_t)(f.group_base + (g < f.n_groups ? g : 0)) * hotw::kEntryWords;
    }
    RL_PART Rec chunk_rec(uint32_t c) const { return recs[min(f.start + c * kHotChunk + lane, f.end - 1)]; }
};

// One key's chain: its state (registers; written to LDS when it changes), the range [T0, T1) in
// which every acquire is denied with remaining 0 (whole chunks and groups inside it are decided
// without being read), the sliding-window allow-time table, and the prefetched chunk.
template <int A_, class Env_>
struct KeyChain {
    static constexpr int A = A_;
    using Env = Env_;
    using Rec = typename Env::Rec;
    Env& e;
    const uint32_t kk;                                // 0: the dominant key, 1: the second
    const uint32_t ow;                                // this key's summary words
    const uint32_t hs;                                // its slot in the LDS image
    const uint64_t tag;
    uint64_t sa, sb, sc;
    int64_t T0 = 0, T1 = 0;
    // Sliding window: the allow-time table of the key's current window W. P(t) (the
    // previous bucket, with its TTL lapse) is the same for every state the key passes
    // through inside W (allows only INCR the current bucket, :114-116), so the first
    // times at which an acquire of 1 or 2 permits is allowed with C = thr_c + lane in the
    // current bucket, thr1 / thr2 (per lane; W + w = not in this window), hold until W
    // ends: the allows of W are then found by integer compares, and [T0, T1) after a
    // change is a table read instead of one lone wave's fp64 chain (the reference's
    // arithmetic is only evaluated where the table is built, each entry verified there
    // by the exact predicate, :158-180).
    int64_t thr_w = INT64_MIN, thr_c = 0;             // table for window thr_w, counts thr_c + lane
    int64_t w_cache = INT64_MIN / 2;                  // the window of the last chunk detailed
    int64_t thr1 = 0, thr2 = 0;
    // The next chunk to detail is prefetched (found from the group summaries once [T0, T1) is
    // known), so its records are in flight while this chunk's results are stored.
    Rec pre;
    uint32_t pre_c = 0;

    RL_PART KeyChain(Env& env, uint32_t k)
        : e(env), kk(k), ow(hotw::key_words(k)), hs((uint32_t)(k ? env.hsl1 : env.hsl0)),
          tag(k ? env.f.tag2 : env.f.tag), sa(uni(env.S.sa[hs])), sb(uni(env.S.sb[hs])), sc(uni(env.S.sc[hs])) {}

    RL_PART bool is_key(const Req& q, bool valid) const { return valid && !q.invalid && q.h == tag; }
    RL_PART bool allowed1(int64_t t) const { return hot_pred_k<A>(e.L, t, sa, sb, sc, 1); }
    RL_PART void store_state() const {
        wave_fence();
        if (e.lane == 0) { e.S.sa[hs] = sa; e.S.sb[hs] = sb; e.S.sc[hs] = sc; }
        wave_fence();
    }
    // T1 from the closed-form guess verified at g - 1; when the guess overshoots (the
    // check fails), the exact first allowed time by a search on the same arithmetic
    RL_PART int64_t t1_of(int64_t t0) const {
        int64_t g = hot_tk_guess<A>(e.L, t0, sa, sb, sc, 1);
        if (g > e.hi + 1) g = e.hi + 1;
        if (g <= t0 + 1) return t0;
        auto pred = [&](int64_t t) { return allowed1(t); };
        if (!pred(g - 1)) return g;
        return wave_first_true(t0, g - 1, e.lane, pred);
    }
    // the exact first time an acquire of one permit is allowed, from T0
    RL_PART int64_t t1_exact() const {
        return wave_first_true(T0, e.hi, e.lane, [&](int64_t t) { return allowed1(t); });
    }
    // the table for window W from the count C on (W, C wave-uniform; state sa, sb, sc)
    RL_PART void thr_build(int64_t W, int64_t C) {
        const DevLimiter& L = e.L;
        const uint64_t c_b = e.dbg.now();
        const int64_t w = L.window_ms;
        // the state after C - (its count in W) allows inside W: every lane's own count
        SW2 s1 = sw_unpack(sa, sb, sc);
        const int64_t cnt = C + (int64_t)e.lane;
        if (s1.b1_start != W) {                      // roll into W (as sw_commit_allows)
            if (s1.b1_start == W - w) { s1.b0_cnt = s1.b1_cnt; s1.b0_off = s1.b1_off; }
            else { s1.b0_cnt = 0; s1.b0_off = 0; }
            s1.b1_start = W;
            s1.b1_off = 0;                           // (alive through W whatever it is)
        }
        s1.b1_cnt = (uint32_t)cnt;
        const uint64_t la = (uint64_t)s1.b1_start;
        const uint64_t lb = (uint64_t)s1.b1_cnt | ((uint64_t)s1.b0_cnt << 32);
        const uint64_t lc = (uint64_t)(uint32_t)s1.b1_off | ((uint64_t)(uint32_t)s1.b0_off << 32);
        const int64_t end = W + w;
        auto first = [&](int64_t q) {                // first t in [W, W + w) allowing q
            auto pred = [&](int64_t t) { return hot_pred_k<kAlgoSW>(L, t, la, lb, lc, q); };
            int64_t g = hot_tk_guess<kAlgoSW>(L, W, la, lb, lc, q);
            g = g < W ? W : g > end ? end : g;
            // the guess is exact but at rounding edges: verify, step, else bisect
            for (int it = 0; it < 2; ++it) {
                if (g > W && pred(g - 1)) --g;
                else if (g < end && !pred(g)) ++g;
                else return g;
            }
            if ((g == W || !pred(g - 1)) && (g == end || pred(g))) return g;
            ++e.dbg.n_bisect;
            int64_t l = W, h = end;                  // pred false below l... true at h
            while (l < h) {
                const int64_t m = l + (h - l) / 2;
                if (pred(m)) h = m; else l = m + 1;
            }
            return l;
        };
        thr1 = cnt + 1 <= L.max_permits ? first(1) : end;
        thr2 = cnt + 2 <= L.max_permits ? first(2) : end;
        thr_w = W;
        thr_c = C;
        e.dbg.add(e.dbg.cyc_build, c_b);
    }
    // does the table hold window W at count C?
    RL_PART bool thr_holds(int64_t W, int64_t C) const { return !(thr_w != W || C < thr_c || C - thr_c > 63); }
    // [T0, T1) for the current state from the table, when it covers it
    RL_PART bool t1_table(int64_t t0, int64_t& t1) const {
        if constexpr (A != kAlgoSW) return false;
        const SW2 s0 = sw_unpack(sa, sb, sc);
        const int64_t W = s0.b1_start, w = e.L.window_ms;
        if (W != thr_w || t0 < W || t0 >= W + w) return false;
        const int64_t k = (int64_t)s0.b1_cnt - thr_c;
        if (k < 0 || k > 63) return false;
        const int64_t T = (int64_t)readlane64((uint64_t)thr1, (uint32_t)k);
        t1 = T > e.hi + 1 ? e.hi + 1 : T;
        if (t1 < t0) t1 = t0;
        return true;
    }
    // [T0, T1) of the current state
    RL_PART void retarget() {
        T0 = hot_t0<A>(e.lo, e.hi, sa, sb, sc);
        if (!t1_table(T0, T1)) T1 = t1_of(T0);
    }
};

// One lane's record of the chunk being detailed and its outcome so far; `changed` and
// `t_fresh` ([T0, T1) is for the current state) are wave-uniform.
struct ChunkLane {
    Req q;
    bool hot = false, pend = false;
    bool oa = false;
    int64_t orem = 0;
    double tk = 0.0;
    bool changed = false, t_fresh = false;
};

// the pending prefix inside [T0, T1): denied, remaining 0
template <class KC>
RL_PART void detail_fast_prefix(const KC& k, ChunkLane& d) {
    const bool fast = d.q.op == (uint32_t)kOpAcquire && d.q.now_ms >= k.T0 && d.q.now_ms < k.T1;
    const uint64_t m = __ballot(d.pend && !fast);
    const uint32_t first = m ? (uint32_t)__builtin_ctzll(m) : 64u;
    if (d.pend && k.e.lane < first) {
        d.orem = 0;
        if (KC::Env::TOK && KC::A == kAlgoTB) d.tk = tb_refill(k.e.L, d.q.now_ms, k.sa, k.sb, k.sc);
        d.pend = false;
    }
}

// token bucket: rounds; each applies the prefix up to the first state change
// (every earlier pending request is denied and leaves the state alone, Lua
// :61-67), so a chunk costs 1 + its allows (the balance is a sequential fp64
// recurrence, Lua :56-63)
template <class KC>
RL_PART void detail_tb(KC& k, ChunkLane& d) {
    using Codec = typename KC::Env::CodecT;
    auto& e = k.e;
    const DevLimiter& L = e.L;
    const uint32_t lane = e.lane;
    const Req& q = d.q;
    if (std::is_same<Codec, CodecC>::value && !__any(d.pend && q.op != (uint32_t)kOpAcquire)) {
        // acquires only (the common case): tb_step in straight-line code. The
        // request time as a double is base + now_rel, exact (integers below 2^53),
        // so elapsed = now - last_refill is one exact subtraction of doubles
        // (Lua :56), the same value as the integer difference converted
        const double td = (double)e.base + (double)(q.now_ms - e.base);
        const double pd = (double)q.permits;
        const double cap = L.capacity, rate = L.rate_per_ms, ttld = (double)L.ttl_ms;
        while (__any(d.pend)) {
            const double tok = __longlong_as_double((long long)k.sa);
            const double lastd = (double)(int64_t)k.sb;
            const bool ex = (k.sc & 1u) != 0;
            const double x = tok + (td - lastd) * rate;          // Lua :57-58
            const double rf = (!ex || td > lastd + ttld) ? cap : (x < cap ? x : cap);
            const bool ok = rf >= pd;                              // Lua :61
            const double nt = ok ? rf - pd : rf;
            const uint64_t mut = __ballot(d.pend && ok);
            const uint32_t fm = mut ? (uint32_t)__builtin_ctzll(mut) : 64u;
            if (d.pend && lane <= fm) {
                d.oa = ok;
                d.orem = d2l(nt);                                 // {allowed, tokens}
                d.tk = nt;
                e.n_allowed += ok ? 1u : 0u;
                d.pend = false;
            }
            if (fm < 64u) {                                        // persist (:62-64)
                // (the lanes after it: the next round, ~20 instructions, decides
                // them; [T0, T1) is derived once the chunk is done)
                k.sa = readlane64((uint64_t)__double_as_longlong(nt), fm);
                k.sb = readlane64((uint64_t)q.now_ms, fm);
                k.sc = 1;
                d.changed = true;
            }
        }
    }
    while (__any(d.pend)) {
        Outcome o{};
        if (d.pend) o = tb_step(L, q.op, q.permits, q.now_ms, k.sa, k.sb, k.sc);
        const uint64_t mut = __ballot(d.pend && o.mutate);
        const uint32_t fm = mut ? (uint32_t)__builtin_ctzll(mut) : 64u;
        if (d.pend && lane <= fm) {
            d.oa = o.allowed;
            d.orem = o.remaining;
            d.tk = o.tokens;
            e.n_allowed += o.allowed ? 1u : 0u;
            d.pend = false;
        }
        if (fm < 64u) {                        // fm is wave-uniform: read lanes
            k.sa = readlane64(o.a, fm);
            k.sb = readlane64(o.b, fm);
            k.sc = readlane64(o.c, fm);
            d.changed = true;
            d.t_fresh = false;
            // the later requests inside the new state's [T0, T1) are denied
            // with remaining 0 by time alone (a key at its limit: the balance
            // stays below 1 for a while after an allow), not by another round
            if (__any(d.pend)) {
                k.retarget();
                d.t_fresh = true;
                ++e.dbg.n_tk;
                detail_fast_prefix(k, d);
            }
        }
    }
}

// Sliding window, acquires of at most 2 permits: the greedy scan on the window's table. The
// na-th allow is the first request at or past T_p(C0 + na); rebuilt when the window fills it.
// (One step per allow, thresholds by readlane: a chain's allows are mostly one per chunk, where
// allow runs through per-lane table reads measured slower.) `in`: this lane's request is
// scanned; c_g: the stamp the scan starts at. Leaves the allows' count and the last one's lane.
template <class KC>
RL_PART void sw_scan_table(KC& k, ChunkLane& d, bool in, int64_t W0, int64_t C0, uint64_t c_g,
                           int64_t& na, uint32_t& last) {
    auto& e = k.e;
    const DevLimiter& L = e.L;
    const uint32_t lane = e.lane;
    const Req& q = d.q;
    int64_t kk = 0;
    bool al = false;
    uint32_t cur = 0;
    for (;;) {
        if (C0 + na - k.thr_c > 63) {     // (wave-uniform) table exhausted
            k.thr_build(W0, C0 + na);
            ++e.dbg.n_tk;
        }
        ++e.dbg.n_sw_it;
        const uint32_t ix = (uint32_t)(C0 + na - k.thr_c);
        const int64_t u1 = (int64_t)readlane64((uint64_t)k.thr1, ix);
        const int64_t u2 = (int64_t)readlane64((uint64_t)k.thr2, ix);
        const bool cnd = in && lane >= cur;
        const uint64_t m = __ballot(cnd && q.now_ms >= (q.permits == 1 ? u1 : u2));
        if (cnd) kk = na;
        if (!m) break;
        const uint32_t fa = (uint32_t)__builtin_ctzll(m);
        if (lane == fa) al = true;
        last = fa;
        ++na;
        cur = fa + 1;
    }
    const uint64_t c_r = e.dbg.lap(e.dbg.cyc_sw[1], c_g);
    // remaining after the request: max - est(C0 + kk (+1)) = the number
    // of q <= 2 with T_q at or before t; 2 or more: the exact estimate
    const int64_t cc = C0 + kk + (al ? 1 : 0);
    const int64_t ixl = cc - k.thr_c;
    const bool tab = ixl >= 0 && ixl <= 63;
    const int src = (int)(tab ? ixl : 0);
    const int64_t v1 = shfl64(k.thr1, src), v2 = shfl64(k.thr2, src);
    if (in) {
        int64_t rem;
        if (tab && q.now_ms < v1) rem = 0;
        else if (tab && q.now_ms < v2) rem = 1;
        else {
            const double t = sw_prev_weighted(q.now_ms, k.sa, k.sb, k.sc, L.window_ms, L.inv_window);
            const int64_t est = d2l(t + (double)cc);
            rem = L.max_permits - est > 0 ? L.max_permits - est : 0;
        }
        d.oa = al;
        d.orem = rem;
        e.n_allowed += al ? 1u : 0u;
        d.pend = false;
    }
    e.dbg.add(e.dbg.cyc_sw[2], c_r);
}

// Sliding window, any permits: per request the largest allowed k (K) by the closed form
// corrected by the exact predicate, then the greedy scan as a fixpoint (wave_apply).
template <class KC>
RL_PART void sw_scan_closed(KC& k, ChunkLane& d, bool in, int64_t C0, int64_t& na, uint32_t& last) {
    auto& e = k.e;
    const DevLimiter& L = e.L;
    const Req& q = d.q;
    const int64_t mx = L.max_permits;
    const uint64_t inm = __ballot(in);
    const double tv = in ? sw_prev_weighted(q.now_ms, k.sa, k.sb, k.sc, L.window_ms, L.inv_window)
                         : 0.0;                                // :174, rounded
    auto est = [&](int64_t n) { return d2l(tv + (double)(C0 + n)); };
    int64_t K = -1;
    if (in) {
        K = mx - (int64_t)q.permits - C0 - (int64_t)tv;      // ~ largest k
        if (K >= 0 && est(K) + q.permits > mx) --K;         // rounding edges
        if (K >= 0 && est(K) + q.permits > mx) --K;
        if (est(K + 1) + q.permits <= mx) ++K;
        if (K < -1) K = -1;
    }
    int64_t kk = 0;
    bool x = in && K >= (int64_t)popc_below(inm);
    for (;;) {
        ++e.dbg.n_sw_it;
        kk = (int64_t)popc_below(__ballot(x) & inm);
        const bool nx = in && K >= kk;
        if (!__any(nx != x)) break;
        x = nx;
    }
    const bool al = x;
    const uint64_t am = __ballot(al);
    na = (int64_t)__popcll(am);
    if (am) last = 63u - (uint32_t)__builtin_clzll(am);
    if (in) {
        const int64_t en = est(al ? kk + 1 : kk);             // after the request
        d.oa = al;
        d.orem = mx - en > 0 ? mx - en : 0;
        e.n_allowed += al ? 1u : 0u;
        d.pend = false;
    }
}

// sliding window: inside one window W the acquires only INCR the current
// bucket (:114-116), so with k allows before it an acquire of p permits at t
// is allowed iff t >= T_p(C0 + k) (C0: the bucket's count before the chunk;
// the estimate is non-increasing in t inside W). The allows follow by a greedy
// scan: the k-th is the first request after the (k-1)-th at or past its
// threshold. Thresholds come from the window's table (p <= 2) or, per request,
// from the closed form. Requests the scan cannot take (another window, before the newest
// bucket, near the epoch, a peek or a reset) run the exact step alone.
template <class KC>
RL_PART void detail_sw(KC& k, ChunkLane& d) {
    auto& e = k.e;
    const DevLimiter& L = e.L;
    const uint32_t lane = e.lane;
    ChainDbg& dbg = e.dbg;
    const Req& q = d.q;
    const int64_t w = L.window_ms;
    while (__any(d.pend)) {
        const uint64_t c_it = dbg.now();
        const uint32_t f0 = (uint32_t)__builtin_ctzll(__ballot(d.pend));
        const int64_t t_f = (int64_t)readlane64((uint64_t)q.now_ms, f0);
        // t_f's window: the last one seen, or one division
        if (!(t_f >= k.w_cache && t_f - k.w_cache < w)) {
            int64_t rr;
            k.w_cache = jdiv(t_f, w, L.inv_window, &rr) * w;
        }
        const int64_t W0 = k.w_cache;
        // (window membership by compares: no per-request division)
        const bool in_w = q.now_ms >= W0 && q.now_ms - W0 < w;
        const bool scan = d.pend && q.op == (uint32_t)kOpAcquire && in_w &&
                          (int64_t)k.sa <= W0 && t_f >= w;
        const uint64_t und = __ballot(d.pend && !scan);
        const uint32_t stop = und ? (uint32_t)__builtin_ctzll(und) : 64u;
        const bool in = scan && lane < stop;
        if (__any(in)) {
            const SW2 s0 = sw_unpack(k.sa, k.sb, k.sc);
            const int64_t C0 = s0.b1_start == W0 ? (int64_t)s0.b1_cnt : 0;
            const bool small = !__any(in && q.permits > 2);
            if (small && !k.thr_holds(W0, C0)) {
                k.thr_build(W0, C0);
                ++dbg.n_tk;
            }
            int64_t na = 0;
            uint32_t last = 0;
            const uint64_t c_g = dbg.lap(dbg.cyc_sw[0], c_it);
            if (small) sw_scan_table(k, d, in, W0, C0, c_g, na, last);
            else sw_scan_closed(k, d, in, C0, na, last);
            const uint64_t c_c = dbg.now();
            if (na > 0) {
                const int64_t t_last = (int64_t)readlane64((uint64_t)q.now_ms, last);
                SWGeo gl{};
                gl.curr_start = W0;
                sw_commit_allows(L, gl, k.sa, k.sb, k.sc, (uint32_t)na, t_last);
                d.changed = true;
            }
            dbg.add(dbg.cyc_sw[3], c_c);
        }
        if (stop < 64u) {
            // the exact step of request `stop` alone (wave-uniform arithmetic)
            const uint32_t op_s = (uint32_t)__builtin_amdgcn_readlane((int)q.op, (int)stop);
            const int32_t p_s = __builtin_amdgcn_readlane(q.permits, (int)stop);
            const int64_t t_s = (int64_t)readlane64((uint64_t)q.now_ms, stop);
            const Outcome o = sw_step_g(L, op_s, p_s, t_s, sw_geo(t_s, L), k.sa, k.sb, k.sc);
            if (lane == stop) {
                d.oa = o.allowed;
                d.orem = o.remaining;
                e.n_allowed += o.allowed ? 1u : 0u;
                d.pend = false;
            }
            if (o.mutate) {
                k.sa = o.a; k.sb = o.b; k.sc = o.c;
                d.changed = true;
                k.thr_w = INT64_MIN;               // P may have changed: rebuild
            }
        }
    }
}

// The key's records of chunk c, one by one (lane = arrival order inside the chunk): the fast
// check against [T0, T1), then the sequential run of the key's state changes. mn_l / mx_l /
// ns_l: this lane's chunk summary in the group being descended; todo_after: the group's chunks
// still to decide after this one.
template <class KC>
RL_PART void detail(KC& k, uint32_t c, int64_t mn_l, int64_t mx_l, uint32_t ns_l, uint64_t todo_after) {
    using Env = typename KC::Env;
    using Codec = typename Env::CodecT;
    constexpr int A = KC::A;
    auto& e = k.e;
    const RegionArgs& a = e.a;
    const HotInfo& f = e.f;
    ChainDbg& dbg = e.dbg;
    ++dbg.n_detail;
    const uint64_t c_det = dbg.now();
    const uint32_t j = f.start + c * kHotChunk + e.lane;
    const bool valid = j < f.end;
    const bool use_pre = k.pre_c == c;
    dbg.n_prehit += use_pre ? 1u : 0u;
    typename Env::Rec r = k.pre;                      // (copied: a reference into k would keep k in memory)
    if (!use_pre) r = e.recs[valid ? j : f.start];
    ChunkLane d;
    d.q = Codec::dec(r, e.base);
    const Req& q = d.q;
    d.hot = k.is_key(q, valid);
    d.tk = __builtin_nan("");
    d.pend = d.hot;
    if (A == kAlgoTB && d.hot && q.op == (uint32_t)kOpAcquire && (int64_t)q.permits > e.L.max_permits) {
        d.orem = kRemUnknown;                       // :110-116, no state access
        d.pend = false;
    }
    detail_fast_prefix(k, d);
    const uint64_t c_run = dbg.lap(dbg.cyc_pre, c_det);
    if constexpr (A == kAlgoTB) detail_tb(k, d);
    else detail_sw(k, d);
    if (d.changed) {
        k.store_state();
        ++dbg.n_changed;
    }
    // [T0, T1) for the next chunks, after every change (measured: leaving it empty
    // through runs of changing chunks read the chunk after each of them needlessly)
    const uint64_t c_srch = dbg.now();
    if (d.t_fresh) {
        // computed after the last change
    } else if (d.changed) {
        k.retarget();
        ++dbg.n_tk;
    } else if (k.T1 < e.hi && __any(d.hot && q.op == (uint32_t)kOpAcquire && q.now_ms >= k.T1)) {
        // no change although requests lay past T1: T1 was only a lower bound of the
        // first allowed time (the guess undershot); without this the chunks up to
        // the real one would all be read and decided one by one. Exact, from T0.
        k.T1 = k.t1_exact();
        ++dbg.n_tk;
    }
    // the next chunk to detail: the first one left in the group that the
    // new [T0, T1) does not decide (else the next chunk); its loads go out now
    {
        const bool skip_l = ns_l == 0 && mn_l >= k.T0 && mx_l < k.T1;
        const uint64_t nx = todo_after & ~__ballot(skip_l);
        k.pre_c = nx ? (c & ~63u) + (uint32_t)__builtin_ctzll(nx) : c + 1;
        k.pre = e.chunk_rec(k.pre_c);
    }
    if (dbg.on) {
        const uint64_t c_end = __builtin_amdgcn_s_memtime();
        dbg.cyc_run += c_srch - c_run;
        dbg.cyc_search += c_end - c_srch;
    }
    if (d.hot && !(RL_ABLATION(a) & kAblNoChainStores)) {
        put_res<typename Env::Res>(a, j, d.oa, d.orem);
        if (Env::TOK) a.tok[j] = d.tk;
    }
    dbg.add(dbg.cyc_detail, c_det);
}

}  // namespace rl
