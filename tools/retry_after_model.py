#!/usr/bin/env python3
"""CPU model of the retry-after search (csrc/rl_retry.hpp `retry_search`) for ONE query: the
exact predicate P(t) restated from csrc/rl_device.hpp (tb_step / sw_step_g / sw_step_cache: would
an acquire of p at millisecond t be allowed on this state, not applied), and around it the
kernel's search step for step: t0, the closed-form guess, its check at guess - 2 .. guess + 2
by the exact predicate, the bisection fallback. It runs on (state, limiter, permits, now) tuples
and counts how often the fallback runs, so a guess that is off, a bound that is short or a loop
that does not end shows up here instead of on the GPU (tests/test_retry_after_model.py checks it
against the oracle). Test tooling only: nothing in the product imports it.

state  TB: {"tokens": float, "last": int ms, "exists": bool}
       SW: {"b1_start", "b1_cnt", "b1_off", "b0_cnt", "b0_off", "x"}: the two newest buckets as a
           slot holds them (b0 starts at b1_start - w; off = last INCR - bucket start) and the
           local cache's block-until ms (0: none)

usage: tools/retry_after_model.py [--n N] [--seed S]
"""
import argparse
import math
import random
from fractions import Fraction

SW, TB = 0, 1
NEVER, INVALID = -1, -2
LF_MUL, LF_FMA = 1, 2


def d2l(d):
    if d != d:
        return 0
    return int(d)


def fma(a, b, c):
    """One correctly rounded a * b + c (exact rational arithmetic, rounded once)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def pct_flags(w):
    """kLfPctMul / kLfPctFma as the engine derives them (rl_engine.cpp pct_flags)."""
    if w > (1 << 22):
        return 0
    inv, dw = 1.0 / float(w), float(w)
    mul = fm = True
    for r in range(1, w):
        dr = float(r)
        exact, q = dr / dw, dr * inv
        if q != exact:
            mul = False
            if fm and fma(fma(-q, dw, dr), inv, q) != exact:
                fm = False
        if not (mul or fm):
            break
    return LF_MUL if mul else LF_FMA if fm else 0


class Lim:
    def __init__(self, algo, max_permits, window_ms, refill_per_s=0.0, cache_ttl_ms=0, lflags=None):
        self.algo, self.max, self.w = algo, int(max_permits), int(window_ms)
        self.ttl = 2 * self.w if algo == TB else self.w
        self.refill_per_s = float(refill_per_s)
        self.rate = refill_per_s / 1000.0
        self.inv_rate = 1.0 / self.rate if self.rate > 0.0 else 0.0
        self.capacity = float(self.max)
        self.inv_w = 1.0 / float(self.w)
        self.cache_ttl = int(cache_ttl_ms) if algo == SW else 0
        self.lflags = pct_flags(self.w) if lflags is None else lflags


# ---------------------------------------------------------------- the exact predicate
def jdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def sw_pct(r, L):
    dr = float(r)
    if L.lflags & LF_MUL:
        return dr * L.inv_w
    if L.lflags & LF_FMA:
        q = dr * L.inv_w
        return fma(fma(-q, float(L.w), dr), L.inv_w, q)
    return dr / float(L.w)


def sw_geo(t, L):
    w = L.w
    q = jdiv(t, w)
    r = t - q * w
    return q * w, jdiv(t - w, w) * w, 1.0 - sw_pct(r, L)


def sw_get(s, start, t, w):
    if s["b1_cnt"] and s["b1_start"] == start and not (t > s["b1_start"] + s["b1_off"] + w):
        return s["b1_cnt"]
    b0 = s["b1_start"] - w
    if s["b0_cnt"] and b0 == start and not (t > b0 + s["b0_off"] + w):
        return s["b0_cnt"]
    return 0


def sw_est(L, t, s):
    """sw_estimate (getCurrentCount, SlidingWindowRateLimiter.java:158-180)."""
    curr_start, prev_start, pw = sw_geo(t, L)
    return d2l(float(sw_get(s, prev_start, t, L.w)) * pw + float(sw_get(s, curr_start, t, L.w)))


def sw_allowed(L, p, t, s):
    """`allowed` of sw_step_g for an acquire."""
    w = L.w
    curr_start = sw_geo(t, L)[0]
    if sw_est(L, t, s) + p > L.max:
        return False
    if s["b1_start"] == curr_start:
        alive = s["b1_cnt"] and not (t > s["b1_start"] + s["b1_off"] + w)
        n = s["b1_cnt"] + 1 if alive else 1
    elif curr_start > s["b1_start"] or (s["b1_cnt"] == 0 and s["b0_cnt"] == 0):
        n = 1
    elif curr_start == s["b1_start"] - w:
        b0 = s["b1_start"] - w
        alive = s["b0_cnt"] and not (t > b0 + s["b0_off"] + w)
        n = s["b0_cnt"] + 1 if alive else 1
    else:
        n = 1
    return n <= L.max


def tb_refill(L, t, s):
    if not (s["exists"] and not (t > s["last"] + L.ttl)):
        return L.capacity
    x = s["tokens"] + float(t - s["last"]) * L.rate
    return x if x < L.capacity else L.capacity


def peek(L, t, s):
    """What getAvailablePermits reads at t on state s (RL_OP_PEEK's remaining): no cache."""
    if L.algo == TB:
        return d2l(tb_refill(L, t, s))
    return max(0, L.max - sw_est(L, t, s))


def pred(L, p, t, s, full=False):
    """P(t): an acquire of p at t is allowed on state s, not applied. `full`: the whole quota is
    available at t (the peek reads max; p and the cache word are not looked at)."""
    if full:
        return peek(L, t, s) == L.max
    if L.algo == TB:
        if p > L.max:
            return False
        return tb_refill(L, t, s) >= float(p)
    if L.cache_ttl > 0 and s["x"] != 0 and t < s["x"]:
        return False
    return sw_allowed(L, p, t, s)


# ---------------------------------------------------------------- the search
def sw_guess_window(W, lo, prev, curr, room, w):
    need = room - curr
    if not (need > 0.0):
        return -1
    t = W
    if prev > 0.0 and not (prev < need):
        rr = float(w) * (1.0 - need / prev)
        t = W + int(rr) + 1
    if t < lo:
        t = lo
    return t if t < W + w else -1


def search(L, p, now, s, stats=None, full=False):
    """The kernel's per-query answer for a key that has a slot (after the permits checks).
    `full`: the wait for the whole quota (rl_quota's reset: p = max, the cache word ignored)."""
    if full:
        p = L.max
    if p <= 0:
        return INVALID
    if p > L.max:
        return NEVER
    w = L.w
    t0 = now
    if L.algo == TB:
        hi = s["last"] + L.ttl + 1
    else:
        if s["b1_cnt"]:
            t0 = max(t0, s["b1_start"] + s["b1_off"])
        elif s["b0_cnt"]:
            t0 = max(t0, s["b1_start"] - w + s["b0_off"])
        if L.cache_ttl > 0 and not full:
            t0 = max(t0, s["x"])
        hi = s["b1_start"] + 2 * w
    if stats is not None:
        stats["queries"] = stats.get("queries", 0) + 1
    if pred(L, p, t0, s, full):
        return t0 - now
    if stats is not None:
        stats["searches"] = stats.get("searches", 0) + 1
    # ---- the guess
    if L.algo == TB:
        d = (float(p) - s["tokens"]) * L.inv_rate
        if math.isfinite(d):
            d = float(math.ceil(d))
        cap = float(L.ttl + 1)
        if not (d < cap):
            d = cap
        if not (d > 0.0):
            d = 0.0
        g = s["last"] + int(d)
    else:
        W1 = sw_geo(t0, L)[0]
        n1 = n0 = 0.0
        E1, E0 = W1 + w - 1, W1 - 1
        if s["b1_start"] == W1:
            if s["b1_cnt"]:
                n1, E1 = float(s["b1_cnt"]), s["b1_start"] + s["b1_off"] + w
            if s["b0_cnt"]:
                n0, E0 = float(s["b0_cnt"]), s["b1_start"] + s["b0_off"]
        elif s["b1_start"] == W1 - w:
            if s["b1_cnt"]:
                n0, E0 = float(s["b1_cnt"]), s["b1_start"] + s["b1_off"] + w
        room = float(L.max - p + 1)
        lo, W2 = t0 + 1, W1 + w
        g = -1
        t = sw_guess_window(W1, lo, n0, n1, room, w)
        if t >= 0 and t <= E0:
            g = t
        if g < 0 and n1 < room:
            t = max(E0 + 1, lo, W1)
            if t < W2:
                g = t
        if g < 0:
            t = sw_guess_window(W2, max(lo, W2), n1, 0.0, room, w)
            g = t if (t >= 0 and t <= E1) else max(E1 + 1, W2)
    if g > hi:
        g = hi
    if g < t0 + 1:
        g = t0 + 1
    # ---- the guess and two neighbours either way, by the exact predicate
    lo_f, hi_t, hi_known = t0, hi, False
    t = g
    if pred(L, p, t, s, full):
        k = 0
        while True:
            if t - 1 == t0 or not pred(L, p, t - 1, s, full):
                return t - now
            t -= 1
            if k == 2:
                break
            k += 1
        hi_t, hi_known = t, True
    else:
        lo_f = t
        k = 0
        while k < 2 and t < hi:
            t += 1
            if pred(L, p, t, s, full):
                return t - now
            lo_f = t
            k += 1
    # ---- bisection on (lo_f: false, hi_t: true)
    if stats is not None:
        stats["bisections"] = stats.get("bisections", 0) + 1
    if not hi_known and not pred(L, p, hi_t, s, full):
        return NEVER
    while hi_t - lo_f > 1:
        mid = lo_f + (hi_t - lo_f) // 2
        if pred(L, p, mid, s, full):
            hi_t = mid
        else:
            lo_f = mid
    return hi_t - now


def scan(L, p, now, s):
    """The definition: the first t >= now with P(t), by a full scan (no monotonicity used; it
    asserts that no denial follows the first allow inside the bound)."""
    if p <= 0:
        return INVALID
    if p > L.max:
        return NEVER
    bound = 2 * L.w + L.cache_ttl + 2
    first = None
    for t in range(now, now + bound + 1):
        ok = pred(L, p, t, s)
        if ok and first is None:
            first = t
        assert ok or first is None, ("not monotone", L.algo, p, now, t, s)
    assert first is not None, ("no allow inside the bound", L.algo, p, now, s)
    return first - now


# ---------------------------------------------------------------- random states
def random_tb(rnd, L, p, now):
    """A bucket written at most ttl + 2 ms ago; a share with the balance within 1 ulp of p
    (before the refill since `last` is added) or exactly on a refill step below it."""
    last = now - rnd.randrange(0, L.ttl + 3)
    r = rnd.random()
    if r < 0.25:
        tok = float(p)
        for _ in range(rnd.randrange(0, 2)):
            tok = math.nextafter(tok, 0.0)
        tok -= float(rnd.randrange(0, 4)) * L.rate * rnd.choice([0, 1, rnd.randrange(1, 50)])
        tok = max(tok, 0.0)
    elif r < 0.35:
        tok = math.nextafter(float(p), rnd.choice([0.0, 1e9]))
    elif r < 0.7:
        tok = rnd.uniform(0.0, float(p))
    else:
        tok = rnd.uniform(0.0, L.capacity)
    return {"tokens": tok, "last": last, "exists": rnd.random() > 0.03}


def random_sw(rnd, L, p, now):
    """Two buckets whose newest INCR is at or before now; a share with the estimate at now at
    max - p or max - p + 1; a cache word when the limiter has the cache."""
    w = L.w
    W = (now // w) * w
    b1_start = W - w * rnd.choice([0, 0, 0, 1, 1, 2])
    hi_off = min(w - 1, now - b1_start)
    b1_off = rnd.randrange(0, hi_off + 1)
    b0_off = rnd.randrange(0, w)
    r = rnd.random()
    tot = L.max - p + rnd.choice([0, 1]) if r < 0.4 else rnd.randrange(0, L.max + 2)
    tot = max(tot, 0)
    b1_cnt = rnd.randrange(0, tot + 1)
    b0_cnt = rnd.choice([tot - b1_cnt, rnd.randrange(0, L.max + 1), 2 * (tot - b1_cnt)])
    s = {"b1_start": b1_start, "b1_cnt": b1_cnt, "b1_off": b1_off, "b0_cnt": b0_cnt,
         "b0_off": b0_off, "x": 0}
    if r < 0.4 and b1_start == W:
        # the estimate at now exactly at max - p or one above it (the decision's threshold)
        n = b1_cnt + (L.max - p + rnd.choice([0, 1]) - sw_est(L, now, s))
        if n >= 0:
            s["b1_cnt"] = b1_cnt = n
    if b1_cnt == 0:
        s["b1_off"] = 0
    if b0_cnt == 0:
        s["b0_off"] = 0
    if L.cache_ttl > 0 and rnd.random() < 0.5:
        # a put of a count >= max at some request time `wr` <= now (x = wr + ttl)
        s["x"] = now - rnd.randrange(0, L.cache_ttl + 3) + L.cache_ttl
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rnd = random.Random(a.seed)
    t0 = 1_700_000_000_000
    lims = [("tb 5 @ 10/s w 1000", Lim(TB, 5, 1000, 10.0)), ("tb 5 @ 0.5/s w 300", Lim(TB, 5, 300, 0.5)),
            ("tb 7 @ 3.3/s w 1000", Lim(TB, 7, 1000, 3.3)), ("sw 10 / 200 ms", Lim(SW, 10, 200)),
            ("sw 10 / 200 ms, cache 50", Lim(SW, 10, 200, 0.0, 50))]
    for name, L in lims:
        stats, bad = {}, 0
        for _ in range(a.n):
            now = t0 + rnd.randrange(0, 10 * L.w)
            p = rnd.randrange(1, L.max + 1)
            s = random_tb(rnd, L, p, now) if L.algo == TB else random_sw(rnd, L, p, now)
            bad += search(L, p, now, s, stats) != scan(L, p, now, s)
        q, se, bi = stats.get("queries", 0), stats.get("searches", 0), stats.get("bisections", 0)
        print(f"{name}: {q} queries, {se} searched, {bi} bisected "
              f"({100.0 * bi / max(1, se):.2f}% of the searches), {bad} mismatches")


if __name__ == "__main__":
    main()
