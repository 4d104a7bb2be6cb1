"""CPU check of the quota lookup's per-query work (tools/quota_model.py, the model of
csrc/rl_quota.hip: peek, reset search, retry search) against the definition of rl_quota evaluated
on the Python oracle: remaining = A(now) and reset = the first t in a FULL scan of
now .. now + 2w + 2 with A(t) == max, where A is max(0, max - _current_count) for a sliding window
and _tb_peek for a token bucket. The scan assumes no monotonicity; it asserts that A never drops
after first reaching max. The GPU code is checked by tests/test_gpu_quota.py; this pins the search
on thresholds: balances within 1 ulp of cap, expiry before refill, window counts 0 / 1 / 2 / max
with and without a live previous bucket, the window's first and last millisecond, a cache word.

It also asserts the identity the reset search rests on (DESIGN.md §4 "Quota queries"): on every
state the reset equals the retry search of p = max with the local cache ignored."""
import importlib.util
import itertools
import math
import os
import random

from oracle.rl_oracle import PyOracle

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("quota_model", os.path.join(_ROOT, "tools", "quota_model.py"))
qm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(qm)
rm = qm.rm

T0 = 1_700_000_000_000
KEY = 12345


def _oracle_for(L, s):
    """A PyOracle holding exactly the model state s of limiter L for KEY (as
    tests/test_retry_after_model.py builds it)."""
    o = PyOracle()
    lid = o.add_limiter(L.algo, L.max, L.w, L.refill_per_s, local_cache_ttl_ms=L.cache_ttl)
    ent = []
    if L.algo == rm.TB:
        if s["exists"]:
            ent.append((lid, KEY, 1, 0, 0, s["tokens"], s["last"], s["last"] + 2 * L.w))
    else:
        if s["b1_cnt"]:
            ent.append((lid, KEY, 0, s["b1_start"], s["b1_cnt"], 0.0, 0, s["b1_start"] + s["b1_off"] + L.w))
        if s["b0_cnt"]:
            b0 = s["b1_start"] - L.w
            ent.append((lid, KEY, 0, b0, s["b0_cnt"], 0.0, 0, b0 + s["b0_off"] + L.w))
        if L.cache_ttl and s["x"]:
            o.cache[(lid, KEY)] = (L.max, s["x"] - L.cache_ttl)      # a put of a count >= max
    o.load_keyspace(ent)
    return o, o.limiters[lid]


def _oracle_quota(L, now, s):
    """(A(now), min{t >= now: A(t) == max} - now) on the oracle, by the full scan."""
    o, OL = _oracle_for(L, s)

    def A(t):
        if L.algo == rm.TB:
            return o._tb_peek(OL, KEY, t)[0]
        return max(0, OL.max_permits - o._current_count(OL, KEY, t))

    first = None
    for t in range(now, now + 2 * L.w + 2 + 1):
        ok = A(t) == L.max
        if ok and first is None:
            first = t
        assert ok or first is None, ("A drops after first reaching max", now, t, s)
    assert first is not None, ("no full quota inside the bound", now, s)
    return A(now), first - now


def _check(L, now, s, stats=None):
    """One state: the model against the oracle, the bound, the identity. Returns the reset."""
    rem, reset, retry = qm.query(L, now, s, stats=stats)
    want_rem, want_reset = _oracle_quota(L, now, s)
    assert (rem, reset) == (want_rem, want_reset), (L.algo, L.max, L.w, now, s, (rem, reset), (want_rem, want_reset))
    assert retry is None and 0 <= reset <= 2 * L.w + 1
    plain = dict(s, x=0) if L.algo == rm.SW else s
    assert reset == rm.search(qm.without_cache(L), L.max, now, plain), ("identity", now, s)
    return reset


# small windows keep the full scan short; the arithmetic classes do not depend on the size
TB_CASES = [
    ("tb 5 @ 100/s w 30", (rm.TB, 5, 30, 100.0), 2500),
    ("tb 5 @ 2/s w 20 (2w * rate < cap: expiry at last + 2w + 1 before refill)", (rm.TB, 5, 20, 2.0), 2500),
    ("tb 7 @ 33.3/s w 25", (rm.TB, 7, 25, 33.3), 2500),
]
# one window of each class of the window fraction (mul, fma, divide), with and without the cache
SW_CASES = [
    ("sw 10 / 25 ms (mul)", (rm.SW, 10, 25), {}),
    ("sw 3 / 50 ms (fma)", (rm.SW, 3, 50), {}),
    ("sw 10 / 37 ms (divide)", (rm.SW, 10, 37), {"lflags": 0}),
    ("sw 4 / 16 ms, cache ttl 30", (rm.SW, 4, 16, 0.0, 30), {}),
    ("sw 10 / 40 ms, cache ttl 10", (rm.SW, 10, 40, 0.0, 10), {}),
]


def test_token_bucket_reset_equals_the_oracle_scan():
    for i, (name, spec, n) in enumerate(TB_CASES):
        L = rm.Lim(*spec)
        rnd = random.Random(300 + i)
        stats, pos, near = {}, 0, 0
        for _ in range(n):
            now = T0 + rnd.randrange(0, 10 * L.w)
            s = qm.random_state(rnd, L, now)
            near += s["exists"] and 0 < L.capacity - s["tokens"] <= 2 * math.ulp(L.capacity)
            pos += _check(L, now, s, stats) > 0
        assert pos >= n // 10 and n - pos >= n // 10, (name, pos, n)
        assert near >= 20, (name, "too few balances within 1 ulp of cap", near)
        assert stats.get("bisections", 0) < 0.05 * max(1, stats.get("searches", 0)), (name, stats)
    # expiry before refill: a drained bucket reads full the millisecond after its hash expires
    L = rm.Lim(rm.TB, 5, 20, 2.0)
    assert 2 * L.w * L.rate < L.capacity
    s = {"tokens": 0.0, "last": T0, "exists": True}
    assert _check(L, T0 + 3, s) == 2 * L.w + 1 - 3
    # exactly one refill step short of cap, and 1 ulp below cap at `last`
    L = rm.Lim(rm.TB, 5, 30, 100.0)
    assert _check(L, T0, {"tokens": 4.9, "last": T0, "exists": True}) == 1
    assert _check(L, T0, {"tokens": math.nextafter(5.0, 0.0), "last": T0, "exists": True}) == 1
    assert _check(L, T0, {"tokens": 5.0, "last": T0, "exists": True}) == 0


def _sw_grid(L):
    """now at window offsets 0, w // 2 and w - 1; the newest bucket in now's window, the one before
    or two before; its count 0 / 1 / 2 / max with the last INCR early and late; the bucket before
    it absent, 1 or max with its last INCR early and late; with a cache word where there is one."""
    w = L.w
    W = (T0 // w + 3) * w
    for now_off, b1_rel, n1, n0, late1, late0 in itertools.product(
            (0, w // 2, w - 1), (0, 1, 2), (0, 1, 2, L.max), (0, 1, L.max), (False, True), (False, True)):
        now = W + now_off
        b1_start = W - b1_rel * w
        b1_off = min(w - 1, now - b1_start) if late1 else 0
        s = {"b1_start": b1_start, "b1_cnt": n1, "b1_off": b1_off if n1 else 0,
             "b0_cnt": n0, "b0_off": (w - 1 if late0 else 0) if n0 else 0, "x": 0}
        yield now, s
        if L.cache_ttl:
            yield now, dict(s, x=now + 1 + (now_off % L.cache_ttl))       # a rejecting entry, live at now


def test_sliding_window_reset_equals_the_oracle_scan():
    for i, (name, spec, kw) in enumerate(SW_CASES):
        L = rm.Lim(*spec, **kw)
        seen = {"zero": 0, "pos": 0, "live_prev": 0, "cache": 0}
        for now, s in _sw_grid(L):
            r = _check(L, now, s)
            seen["pos" if r > 0 else "zero"] += 1
            seen["live_prev"] += r > 0 and s["b0_cnt"] > 0 and s["b1_start"] == (now // L.w) * L.w
            if s["x"]:
                seen["cache"] += 1
                # the cache word delays an acquire, never the quota
                assert r == qm.query(L, now, dict(s, x=0))[1]
        assert seen["zero"] >= 20 and seen["pos"] >= 100 and seen["live_prev"] >= 20, (name, seen)
        assert (seen["cache"] > 0) == (L.cache_ttl > 0)
        rnd = random.Random(400 + i)
        stats = {}
        for _ in range(1200):
            now = T0 + rnd.randrange(0, 10 * L.w)
            _check(L, now, qm.random_state(rnd, L, now), stats)
        assert stats.get("searches", 0) >= 60, (name, stats)
        assert stats.get("bisections", 0) < 0.05 * stats["searches"], (name, stats)


def test_a_cache_word_changes_retry_but_not_reset():
    L = rm.Lim(rm.SW, 4, 16, 0.0, 30)
    W = (T0 // 16) * 16
    s = {"b1_start": W, "b1_cnt": 1, "b1_off": 2, "b0_cnt": 0, "b0_off": 0, "x": W + 2 + 30}
    now = W + 5
    rem, reset, retry = qm.query(L, now, s, p=1)
    assert (rem, reset) == _oracle_quota(L, now, s)
    assert rem == 3 and retry == s["x"] - now            # room for 1, but the entry rejects until x
    assert qm.query(L, now, dict(s, x=0), p=1) == (rem, reset, 0)
    assert reset == 16 + 1 - 5           # one ms into the next window a count of 1 weighs less than 1
    assert rm.search(L, L.max, now, s) != reset           # retry-after of max counts the cache


def test_retry_part_skip_invalid_and_absent():
    L = rm.Lim(rm.TB, 5, 1000, 10.0)
    s = {"tokens": 0.0, "last": T0, "exists": True}
    assert qm.query(L, T0, s) == (0, 500, None)
    assert qm.query(L, T0, s, p=3) == (0, 500, rm.search(L, 3, T0, s)) == (0, 500, 300)
    assert qm.query(L, T0, s, p=6) == (0, 500, qm.NEVER)
    assert qm.query(L, T0, s, p=3, skip=True) == (0, 500, 0)
    assert qm.query(L, T0, s, p=0, skip=True) == (0, 500, 0)      # a skipped query's permits is not looked at
    assert qm.query(L, T0, s, p=0) == (qm.INVALID,) * 3 == qm.query(L, T0, s, p=-3)
    assert qm.query(L, T0 + 50, None, p=5) == (5, 0, 0)           # no slot: the full quota
    assert qm.query(L, T0 + 2001, s, p=5) == (5, 0, 0)            # the hash expired
    S = rm.Lim(rm.SW, 10, 200)
    assert qm.query(S, T0, None, p=11) == (10, 0, qm.NEVER)
    full = {"b1_start": T0, "b1_cnt": 10, "b1_off": 20, "b0_cnt": 0, "b0_off": 0, "x": 0}
    assert qm.query(S, T0 + 30, full, p=10) == (0, 191, 191)      # 20 + 200 + 1 - 30: the PEXPIRE lapses


def test_bisection_fallback_is_exact(monkeypatch):
    """With the guesses disabled every reset search ends in the bisection: same answers."""
    monkeypatch.setattr(rm, "sw_guess_window", lambda W, lo, prev, curr, room, w: -1)
    rnd = random.Random(9)
    for L in (rm.Lim(rm.TB, 5, 30, 100.0), rm.Lim(rm.SW, 10, 25), rm.Lim(rm.SW, 4, 16, 0.0, 30)):
        L.inv_rate = 0.0                                 # the token-bucket guess becomes `last`
        stats = {}
        for _ in range(800):
            now = T0 + rnd.randrange(0, 10 * L.w)
            s = qm.random_state(rnd, L, now)
            rem, reset, _ = qm.query(L, now, s, stats=stats)
            assert (rem, reset) == _oracle_quota(L, now, s), (now, s)
        assert stats.get("bisections", 0) > 30, stats
