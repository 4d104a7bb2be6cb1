// rl_hot_walk.hpp — the hot chains' allow walk (`walk`): a key at its limit decided from its
// state and k_hot_summ's per-ms table instead of chunk by chunk. Included by rl_hot.hpp.
#pragma once
#include "rl_hot_detail.hpp"

#pragma clang fp contract(off)

namespace rl {

// The table window: lane l holds ms wb + l (A), wb + 64 + l (B), wb + 128 + l (C, in flight) of
// the key's per-ms table (the first plain acquire of 1 / of at most 2 permits in each ms).
struct WalkTable {
    const uint2* wt;
    uint32_t span;                                    // the batch's ms
    int64_t lo;
    uint32_t lane;
    int64_t wb;
    uint2 tA, tB, tC;
    RL_PART uint2 at(int64_t t) const { return wt[min((uint32_t)(t - lo), span - 1u)]; }
    RL_PART void fill(int64_t b) {
        wb = b;
        tA = at(wb + lane); tB = at(wb + 64 + lane); tC = at(wb + 128 + lane);
    }
    // ts into view A
    RL_PART void seek(int64_t ts) {
        if (ts < wb || ts >= wb + 192) {              // far ahead (or searched again
                                                      // after a special): refill the window
            fill(lo + ((ts - lo) & ~(int64_t)63));
        }
        while (ts >= wb + 64) {
            wb += 64; tA = tB; tB = tC; tC = at(wb + 128 + lane);
        }
    }
};

// The group window: lane l holds group gwb + l's summary (max plain time, flags, rest word).
struct WalkGroups {
    uint32_t gwb = kNone, g_w2 = 0;
    int64_t g_mx = INT64_MIN;
    uint64_t g_w3 = 0;
    template <class KC>
    RL_PART void load(const KC& k, uint32_t g) {
        if ((g & ~63u) == gwb) return;
        gwb = g & ~63u;
        const bool has = gwb + k.e.lane < k.e.f.n_groups;
        const uint64_t* sg = k.e.grp_at(has ? gwb + k.e.lane : 0u) + k.ow;
        g_mx = has ? (int64_t)sg[1] : INT64_MIN;
        g_w2 = has ? (uint32_t)sg[2] : 0u;
        g_w3 = has ? sg[3] : 0ULL;
    }
};

// The register block: lane l holds chunk cb + l's summary and its pending verdict (vF: the
// register form of rl_hot_words.hpp; vA, vB, vC: the state it is decided under). The verdicts
// are stored when the cursor leaves the block. (The block after it is loaded on entry, so that
// it is in registers when the cursor gets there.)
struct WalkBlock {
    uint32_t cb = kNone, b_w2 = 0, vF = 0;
    int64_t b_mx = INT64_MIN;
    uint64_t vA = 0, vB = 0, vC = 0;
    uint32_t nb = kNone, n_w2 = 0;
    int64_t n_mx = INT64_MIN;
    template <class KC>
    RL_PART void flush(const KC& k) const {
        const uint32_t c = cb + k.e.lane;
        if (cb != kNone && vF != 0 && c < k.e.f.n_chunks && hotw::chunk_n_hot(b_w2)) {
            uint64_t* sm = k.e.summ_at(c) + k.ow;
            sm[0] = vA; sm[1] = vB; sm[2] = vC;
            sm[3] = hotw::reg_to_word(vF, hotw::chunk_n_rest(b_w2));
        }
    }
    template <class KC>
    RL_PART static void load_blk(const KC& k, uint32_t b, uint32_t& w2, int64_t& mx) {
        const uint32_t c = b + k.e.lane;
        const bool has = c < k.e.f.n_chunks;
        const uint64_t* sm = k.e.summ_at(has ? c : 0u) + k.ow;
        w2 = has ? (uint32_t)sm[2] : 0u;
        mx = has ? (int64_t)sm[1] : INT64_MIN;
    }
    template <class KC>
    RL_PART void enter(const KC& k, uint32_t b) {
        if (b == cb) return;
        flush(k);
        cb = b;
        if (b == nb) { b_w2 = n_w2; b_mx = n_mx; }
        else { load_blk(k, b, b_w2, b_mx); ++k.e.dbg.n_enter; }
        vF = 0;
        nb = b + 64;
        load_blk(k, nb, n_w2, n_mx);
    }
    // chunk c's counts word and max plain time (its block entered)
    template <class KC>
    RL_PART void cinfo(const KC& k, uint32_t c, uint32_t& w2, int64_t& mxc) {
        enter(k, c & ~63u);
        w2 = (uint32_t)__builtin_amdgcn_readlane((int)b_w2, (int)(c - cb));
        mxc = (int64_t)readlane64((uint64_t)b_mx, c - cb);
    }
    // the verdict of a denied chunk of the block (this lane's): remaining 0 when its acquires
    // all precede q1
    RL_PART uint32_t deny_fl(int64_t q1) const {
        return b_mx < q1 ? hotw::reg_threshold(hotw::chunk_n_early(b_w2) != 0u) : hotw::reg_walk_denied();
    }
};

// Can the key be walked? Needs its table built (walk_table_on) and its plain acquires in time
// order with at most 2 permits (k_hot_summ's group flags, and the groups' time ranges against
// each other). Sets any_hot as the group descent does.
template <class KC>
RL_PART bool walk_eligible(KC& k) {
    auto& e = k.e;
    const uint32_t lane = e.lane;
    if (!walk_table_on(e.a, e.i, e.f, e.L, e.lo, e.hi)) return false;
    if constexpr (KC::A == kAlgoSW) {
        if (e.lo < e.L.window_ms) return false;           // near the epoch (:170-172)
        if ((int64_t)k.sa > e.lo) return false;           // the state is newer than the batch
    }
    auto up64 = [&](int64_t v, uint32_t o) { return shfl64(v, lane >= o ? (int)(lane - o) : (int)lane); };
    int64_t carry = INT64_MIN;
    for (uint32_t g0 = 0; g0 < e.f.n_groups; g0 += 64) {
        const uint32_t g = g0 + lane;
        const bool has = g < e.f.n_groups;
        const uint64_t* sg = e.grp_at(g) + k.ow;
        const int64_t mn = has ? (int64_t)sg[0] : INT64_MAX;
        const int64_t mx = has ? (int64_t)sg[1] : INT64_MIN;
        const uint32_t w2 = has ? (uint32_t)sg[2] : 0u;
        e.any_hot |= hotw::group_has_hot(w2);
        if (__any(hotw::group_walk_flags(w2))) return false;
        int64_t pmx = mx;                         // max over the groups up to mine
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const int64_t y = up64(pmx, o);
            if (lane >= o && y > pmx) pmx = y;
        }
        int64_t before = up64(pmx, 1);
        if (lane == 0) before = INT64_MIN;
        if (carry > before) before = carry;
        if (__any(mn != INT64_MAX && mn < before)) return false;
        const int64_t top = (int64_t)readlane64((uint64_t)pmx, 63);
        if (top > carry) carry = top;
    }
    return true;
}

// chunks [c0, c1) denied under (x0, x1, x2): whole groups outside the register block
// whose acquires all precede q1 take group verdicts, 64 groups per store
template <class KC>
RL_PART void walk_deny(const KC& k, WalkBlock& blk, WalkGroups& grp, uint32_t c0, uint32_t c1,
                       uint64_t x0, uint64_t x1, uint64_t x2, int64_t q1) {
    const uint32_t lane = k.e.lane;
    while (c0 < c1) {
        const uint32_t b = c0 & ~63u;
        if (c0 == b && c1 >= b + 64 && b != blk.cb) {
            const uint32_t G0 = b / 64, G1 = min(c1 / 64, (b & ~4095u) / 64 + 64);
            grp.load(k, G0);
            const uint32_t g = grp.gwb + lane;
            const bool in = g >= G0 && g < G1;
            const uint64_t bad = __ballot(in && !(grp.g_mx < q1 && !hotw::group_has_special(grp.g_w2) && g * 64 != blk.cb));
            const uint32_t stop = bad ? grp.gwb + (uint32_t)__builtin_ctzll(bad) : G1;
            if (in && g < stop && hotw::group_has_hot(grp.g_w2)) {
                uint64_t* sg = k.e.grp_at(g) + k.ow;
                sg[0] = x0; sg[1] = x1; sg[2] = x2;
                sg[3] = hotw::group_verdict(grp.g_w3, hotw::group_has_early(grp.g_w2));
            }
            if (stop > G0) { c0 = stop * 64; continue; }
        }
        const uint32_t e = min(c1, b + 64);
        blk.enter(k, b);
        const uint32_t c = blk.cb + lane;
        const uint32_t fl = blk.deny_fl(q1);
        if (c >= c0 && c < e) { blk.vA = x0; blk.vB = x1; blk.vC = x2; blk.vF = fl; }
        c0 = e;
    }
}

// the first chunk >= from holding a peek / reset of the key (group flags first)
template <class KC>
RL_PART uint32_t walk_first_special(const KC& k, WalkGroups& grp, uint32_t from) {
    const HotInfo& f = k.e.f;
    const uint32_t lane = k.e.lane;
    for (uint32_t G = from / 64; G < f.n_groups;) {
        grp.load(k, G);
        const uint32_t g = grp.gwb + lane;
        const uint64_t m = __ballot(g >= G && g < f.n_groups && hotw::group_has_special(grp.g_w2));
        if (!m) { G = grp.gwb + 64; continue; }
        const uint32_t gs = grp.gwb + (uint32_t)__builtin_ctzll(m);
        const uint32_t c = gs * 64 + lane;
        const uint64_t* sm = k.e.summ_at(c < f.n_chunks ? c : 0u) + k.ow;
        const uint32_t w2 = c < f.n_chunks ? (uint32_t)sm[2] : 0u;
        const uint64_t mm = __ballot(c >= from && hotw::chunk_n_special(w2));
        if (mm) return gs * 64 + (uint32_t)__builtin_ctzll(mm);
        G = gs + 1;
    }
    return kNone;
}

// The latest ms of the key's plain acquires in the chunks before c (INT64_MIN: none),
// from the records themselves (the summaries of decided chunks hold verdicts by
// now). Plain acquires are in time order (k_hot_summ's flags), so it is the last
// one found going back. Only after a chunk whose key records are specials alone.
template <class KC>
RL_PART int64_t walk_plain_before(const KC& k, uint32_t c) {
    using Codec = typename KC::Env::CodecT;
    const auto& e = k.e;
    for (uint32_t n = c; n-- > 0;) {
        const uint32_t j = e.f.start + n * kHotChunk + e.lane;
        const bool valid = j < e.f.end;
        const Req q = Codec::dec(e.recs[valid ? j : e.f.start], e.base);
        const bool plain = k.is_key(q, valid) && q.op == (uint32_t)kOpAcquire &&
                           !(KC::A == kAlgoTB && (int64_t)q.permits > e.L.max_permits);
        const uint64_t m = __ballot(plain);
        if (m) return uni((int64_t)readlane64((uint64_t)q.now_ms, 63u - (uint32_t)__builtin_clzll(m)));
    }
    return INT64_MIN;
}

// ---- Allow walk. A key at its limit is allowed about once per refill interval (TB) or
// per decay step of its estimate (SW); detailing the chunk of every such allow cost a
// lone wave ~3.6K cycles (mixed_tenants: ~6000 allows per key and batch). The walk
// finds each next allow from the key's state alone: the first ms t >= ts at which the
// key's first plain acquire asking for at most q(t) permits exists — q(t) being what
// the state grants at t (TB: the refilled balance, Lua :56-61, one lane per ms; SW: the
// window's allow-time table, :104) — 64 ms per step with k_hot_summ's per-ms table (the
// first acquire of 1 and of at most 2 permits) in registers. Chunks are decided by verdicts
// k_hot_fill applies: every record of the key denied under the chunk's state but up to 4
// allowed (offsets), the records after each under the state it leaves; chunks (or whole
// groups) whose acquires all precede the first ms the state grants take the chains'
// remaining-0 verdict. The verdicts of the cursor's block of 64 chunks are kept in registers
// and stored when the cursor leaves it. A chunk holding a peek / reset, a fifth allow, or an
// allow after which the next request of the same ms could be allowed too (a burst) is detailed
// as before. Needs the key's plain acquires in time order with at most 2 permits (k_hot_summ's
// group flags); tools/walk_model.py is a CPU model of this loop. False: the key is not walked
// (nothing done). The loop's own scalars stay locals of this function, with the helpers that
// write them (detail_at, undo_cursor, spin), so that their uni() re-declarations stay as they are.
template <class KC>
RL_PART bool walk(KC& k) {
    constexpr int A = KC::A;
    auto& e = k.e;
    const RegionArgs& a = e.a;
    const HotInfo& f = e.f;
    const DevLimiter& L = e.L;
    const uint32_t lane = e.lane;
    const int64_t lo = e.lo, hi = e.hi;
    ChainDbg& dbg = e.dbg;
    if (!walk_eligible(k)) return false;
    const uint32_t span = (uint32_t)(hi - lo) + 1u;
    WalkTable tw{a.walk_tab + (size_t)(2 * e.i + k.kk) * walk_stride(lo, hi), span, lo, lane};
    tw.fill(lo);
    WalkGroups grp;
    WalkBlock blk;
    uint32_t cc = 0;                                  // cursor: chunks before it are decided
    uint64_t ka = k.sa, kb = k.sb, kc = k.sc;         // the state at cc's start
    uint32_t pc = 0, pofs = 0;                        // cc's walked allows: count, offsets
    int64_t ts = lo;                                  // the next allow is at ms >= ts
    bool must = false;                                // cc must be detailed (see detail_at)
    // the latest ms of the key's plain acquires in the chunks detail_at has passed
    // (the boundary ms whose later acquires the table cannot show; INT64_MIN: none)
    int64_t mlast = INT64_MIN;
    int64_t W = 0;                                    // SW: the window of the thresholds in use
    if constexpr (A == kAlgoSW) {
        int64_t rr;
        W = uni(jdiv(ts, L.window_ms, L.inv_window, &rr) * L.window_ms);
    }
    // A bound no correct walk reaches (every step moves the cursor chunk or ts forward):
    // past it the walk stops and flags the batch (RL_E_CAPACITY) instead of spinning.
    uint32_t guard = 4u * (span + f.n_chunks) + 4096u;
    auto spin = [&]() {
        if (guard != 0) --guard;
        return guard == 0;
    };
    // a chunk detailed from the current state (the group descent's path), then the cursor past it
    auto detail_at = [&](uint32_t c) {
        k.retarget();
        detail(k, c, INT64_MAX, INT64_MIN, 1u, 0ULL);
        k.sa = uni(k.sa); k.sb = uni(k.sb); k.sc = uni(k.sc);
        uint32_t w2;
        int64_t mxc;
        blk.cinfo(k, c, w2, mxc);
        cc = c + 1; ka = k.sa; kb = k.sb; kc = k.sc; pc = 0; pofs = 0;
        const bool special = hotw::chunk_n_special(w2) != 0u;
        // the boundary: this chunk's last plain acquire, else (specials only) the last
        // one before it; a chunk without the key's records (reached as a `must` chunk
        // right after the boundary's own) leaves it as it is
        if (mxc != INT64_MIN) mlast = mxc;
        else if (special) mlast = walk_plain_before(k, c);
        mlast = uni(mlast);
        if (special) {
            // a reset may grant acquires the old state denied: the search starts again
            // right after the boundary (every later plain acquire is at or after it)
            ts = mlast == INT64_MIN ? lo : mlast + 1;
        } else if (mlast != INT64_MIN && mlast + 1 > ts) {
            ts = mlast + 1;
        }
        // the next chunks' acquires in the boundary ms come after every table entry of
        // that ms: while the state grants there, the next chunk is detailed too
        must = mlast != INT64_MIN && uni((uint32_t)k.allowed1(mlast)) != 0u;
    };
    // back to the cursor chunk's start state, to detail it (the detail counts its
    // walked allows again)
    auto undo_cursor = [&]() {
        if (lane == 0) e.n_allowed -= pc;
        k.sa = ka; k.sb = kb; k.sc = kc;
    };
    // (every chunk to detail goes through one call site: `detail` is inlined, and a
    // copy per call site made the kernel's code several times larger)
    uint32_t dc = kNone;
    uint32_t spn = walk_first_special(k, grp, 1);     // the next special after the cursor
    const uint64_t c_w0 = dbg.now();
    for (;;) {
        // (the loop-carried scalars re-declared uniform: a value the compiler cannot
        // prove uniform turns every branch on it into an exec-mask region)
        dc = uni(dc); cc = uni(cc); pc = uni(pc); pofs = uni(pofs); ts = uni(ts);
        tw.wb = uni(tw.wb); guard = uni(guard); spn = uni(spn); blk.cb = uni(blk.cb); blk.nb = uni(blk.nb);
        grp.gwb = uni(grp.gwb); must = uni((uint32_t)must) != 0u;
        ka = uni(ka); kb = uni(kb); kc = uni(kc); k.sa = uni(k.sa); k.sb = uni(k.sb); k.sc = uni(k.sc);
        if constexpr (A == kAlgoSW) W = uni(W);
        if (dc != kNone) { detail_at(dc); dc = kNone; }
        if (cc >= f.n_chunks || spin()) break;
        if (spn <= cc) spn = walk_first_special(k, grp, cc + 1);   // (kNone is above every chunk)
        // the cursor chunk: detailed when it must be or holds a special
        if (pc == 0) {
            uint32_t w2;
            int64_t mxc;
            blk.cinfo(k, cc, w2, mxc);
            if (must || hotw::chunk_n_special(w2)) { must = false; dc = cc; continue; }
        }
        // The common path as a loop of its own (find, verdicts, allow: the cursor chunk
        // always holds a walked allow here), so that the register allocator weighs the
        // values it uses above the rest of the chain's; anything else leaves it.
        bool done = false;
        for (;;) {
            cc = uni(cc); pc = uni(pc); pofs = uni(pofs); ts = uni(ts); blk.cb = uni(blk.cb);
            ka = uni(ka); kb = uni(kb); kc = uni(kc); k.sa = uni(k.sa); k.sb = uni(k.sb); k.sc = uni(k.sc);
            // the next allow: the first ms >= ts with an acquire the state grants; q1: the
            // first ms >= ts the state grants anything at
            int64_t tf = INT64_MIN, q1 = INT64_MAX;
            uint32_t rf = 0, pf = 1;
            const uint64_t c_f0 = dbg.now();
            for (;;) {
                ++dbg.n_find;
                ts = uni(ts); tw.wb = uni(tw.wb); guard = uni(guard); q1 = uni(q1);
                if (ts > hi || spin()) break;
                tw.seek(ts);
                int64_t lim_t = hi;                           // SW: the window's end - 1
                int64_t Q1 = 0, Q2 = 0;                       // SW: the window's thresholds
                if constexpr (A == kAlgoSW) {
                    const int64_t w = L.window_ms;
                    if (!(ts >= W && ts - W < w)) {
                        int64_t rr;
                        W = uni(jdiv(ts, w, L.inv_window, &rr) * w);
                    }
                    const SW2 s0 = sw_unpack(k.sa, k.sb, k.sc);
                    const int64_t C = s0.b1_start == W ? (int64_t)s0.b1_cnt : 0;
                    if (!k.thr_holds(W, C)) { k.thr_build(W, C); ++dbg.n_tk; }
                    Q1 = (int64_t)readlane64((uint64_t)k.thr1, (uint32_t)(C - k.thr_c));
                    Q2 = (int64_t)readlane64((uint64_t)k.thr2, (uint32_t)(C - k.thr_c));
                    if (W + w - 1 < lim_t) lim_t = W + w - 1;
                }
                // one 64-ms view: what the state grants per ms (q), the first candidate
                auto view = [&](int64_t tb, const uint2 ent) -> bool {
                    const int64_t t = tb + (int64_t)lane;
                    uint32_t q;
                    if constexpr (A == kAlgoTB) {
                        // tb_refill per lane, its elapsed time as (tb - last) + lane (exact:
                        // integers below 2^53), no contraction (Lua :56-58)
                        const int64_t last = (int64_t)k.sb;
                        const double el = (double)(tb - last) + (double)lane;
                        const double x = __longlong_as_double((long long)k.sa) + el * L.rate_per_ms;
                        double bal = x < L.capacity ? x : L.capacity;
                        if (!(k.sc & 1u) || t > last + L.ttl_ms) bal = L.capacity;
                        q = bal >= 2.0 ? 2u : bal >= 1.0 ? 1u : 0u;
                    } else {
                        q = t >= Q2 ? 2u : t >= Q1 ? 1u : 0u;
                    }
                    if (!(t >= ts && t <= lim_t)) q = 0;
                    const uint64_t mq = __ballot(q != 0);
                    if (mq && q1 == INT64_MAX) q1 = tb + (int64_t)__builtin_ctzll(mq);
                    const uint32_t cnd = q >= 2u ? ent.y : q == 1u ? ent.x : kWalkNone;
                    const uint64_t m = __ballot(cnd != kWalkNone);
                    if (!m) return false;
                    const uint32_t l = (uint32_t)__builtin_ctzll(m);
                    rf = (uint32_t)__builtin_amdgcn_readlane((int)cnd, (int)l);
                    const uint32_t ex = (uint32_t)__builtin_amdgcn_readlane((int)ent.x, (int)l);
                    pf = rf != ex ? 2u : 1u;                  // (q >= 2 and a 2-permit acquire first)
                    tf = tb + (int64_t)l;
                    return true;
                };
                if (view(tw.wb, tw.tA) || view(tw.wb + 64, tw.tB)) break;
                ts = lim_t < tw.wb + 127 ? lim_t + 1 : tw.wb + 128;  // (SW: the next window)
            }
            dbg.add(dbg.cyc_find, c_f0);
            // (no allow before the batch ends: the rest is denied, up to the next special)
            const uint32_t cs = tf == INT64_MIN ? f.n_chunks - 1u : rf / kHotChunk;
            const uint32_t cfl = hotw::reg_walk_allows(pc, pofs);   // cc's verdict, pc > 0
            const uint64_t c_c0 = dbg.now();
            if (spn <= cs || tf == INT64_MIN) {               // a special in (cc, cs] / the end
                blk.enter(k, cc & ~63u);
                const uint32_t fl = pc ? cfl : blk.deny_fl(q1);
                if (blk.cb + lane == cc) { blk.vA = ka; blk.vB = kb; blk.vC = kc; blk.vF = fl; }
                const uint32_t end = spn <= cs ? spn : f.n_chunks;
                walk_deny(k, blk, grp, cc + 1, end, k.sa, k.sb, k.sc, q1);
                if (end == f.n_chunks) { done = true; break; }
                dc = spn;
                break;
            }
            if (cs < cc) {
                // a table entry in a decided chunk: the search bound (ts above every
                // plain acquire before the cursor) excludes it, so this is a logic
                // error; the batch reports RL_E_INTERNAL and the cursor is detailed
                ++e.n_internal;
                if (pc > 0) undo_cursor();
                dc = cc;
                break;
            }
            if (cs == cc && pc > 0) {                         // another allow in the cursor chunk
                if (pc == 4) { undo_cursor(); dc = cc; break; }
            } else if (cs > cc) {
                const uint32_t fl = pc ? cfl : blk.deny_fl(q1);
                if (cc >= blk.cb && cs < blk.cb + 64) {       // (the common case: one block)
                    const uint32_t c = blk.cb + lane;
                    const uint32_t dfl = blk.deny_fl(q1);
                    if (c == cc) { blk.vA = ka; blk.vB = kb; blk.vC = kc; blk.vF = fl; }
                    else if (c > cc && c < cs) { blk.vA = k.sa; blk.vB = k.sb; blk.vC = k.sc; blk.vF = dfl; }
                } else {
                    blk.enter(k, cc & ~63u);
                    const uint32_t fl2 = pc ? cfl : blk.deny_fl(q1);
                    if (blk.cb + lane == cc) { blk.vA = ka; blk.vB = kb; blk.vC = kc; blk.vF = fl2; }
                    walk_deny(k, blk, grp, cc + 1, cs, k.sa, k.sb, k.sc, q1);
                }
                cc = cs; ka = k.sa; kb = k.sb; kc = k.sc; pc = 0; pofs = 0;
            }
            const uint64_t c_a0 = dbg.lap(dbg.cyc_close, c_c0);
            pofs = hotw::reg_offsets_add(pofs, pc, rf % kHotChunk);
            ++pc;
            // the allow (Lua :61-64 / SlidingWindowRateLimiter :114-116) at ms tf
            bool burst;
            if constexpr (A == kAlgoTB) {
                const double nt = uni(tb_refill(L, tf, k.sa, k.sb, k.sc) - (double)pf);
                k.sa = (uint64_t)__double_as_longlong(nt);
                k.sb = (uint64_t)tf;
                k.sc = 1;
                burst = nt >= 1.0;                            // (elapsed 0: the balance is nt)
            } else {
                SWGeo gl{};
                gl.curr_start = W;
                sw_commit_allows(L, gl, k.sa, k.sb, k.sc, 1u, tf);
                k.sa = uni(k.sa); k.sb = uni(k.sb); k.sc = uni(k.sc);
                // the window's table at the new count, when it holds it
                const int64_t C = (int64_t)sw_unpack(k.sa, k.sb, k.sc).b1_cnt;
                if (k.thr_holds(W, C))
                    burst = tf >= (int64_t)readlane64((uint64_t)k.thr1, (uint32_t)(C - k.thr_c));
                else
                    burst = k.allowed1(tf);
            }
            if (lane == 0) ++e.n_allowed;
            ++dbg.n_changed;
            ++dbg.n_walk;
            ts = tf + 1;
            dbg.add(dbg.cyc_allow, c_a0);
            if (burst) {                                      // the next request of ms tf too: detail
                undo_cursor();
                dc = cc;
                break;
            }
        }
        if (done) break;
    }
    blk.flush(k);
    if (guard == 0) ++e.n_internal;                  // the step bound: a walk that would not end
    dbg.add(dbg.cyc_walk, c_w0);
    k.store_state();
    return true;
}

}  // namespace rl
