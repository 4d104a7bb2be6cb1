"""CPU check of the retry-after search (tools/retry_after_model.py, the model of
csrc/rl_retry.hip's per-query search: guess, its check at +-2 by the exact predicate, bisection
fallback) against the definition of rl_retry_after evaluated on the Python oracle: the first
millisecond t in a FULL scan of now .. now + 2w + ttl + 2 at which one acquire on a copy of
the oracle's state is allowed. The scan uses no monotonicity; it asserts that no denial follows
the first allow. The GPU code is checked by tests/test_gpu_retry_after.py; this pins the
search itself on thresholds: balances within 1 ulp of p, estimates at max - p and max - p + 1,
every rounding class of the window fraction, the local cache, expiry before refill."""
import importlib.util
import os
import random

import pytest

from oracle.rl_oracle import PyOracle

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("retry_after_model",
                                               os.path.join(_ROOT, "tools", "retry_after_model.py"))
rm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rm)

T0 = 1_700_000_000_000
KEY = 12345


def _oracle_for(L, s):
    """A PyOracle holding exactly the model state s of limiter L for KEY."""
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


def _oracle_scan(L, p, now, s):
    """min{t >= now: one acquire at t on a copy of the state is allowed} - now, full scan."""
    if p > L.max:
        return rm.NEVER
    o, OL = _oracle_for(L, s)
    kv, exp, cache = dict(o.redis.kv), dict(o.redis.exp), dict(o.cache)
    first = None
    for t in range(now, now + 2 * L.w + L.cache_ttl + 2 + 1):
        if L.algo == rm.TB:
            ok = o._tb_acquire(OL, KEY, p, t)[0]
        else:
            ok = o._sw_acquire(OL, KEY, p, t)[0]
        o.redis.kv, o.redis.exp, o.cache = dict(kv), dict(exp), dict(cache)   # the copy, undone
        if ok and first is None:
            first = t
        assert ok or first is None, ("a denial after the first allow", p, now, t, s)
    assert first is not None, ("no allow inside the bound", p, now, s)
    return first - now


def _run(name, L, n, seed):
    rnd = random.Random(seed)
    stats, bad = {}, []
    gen = rm.random_tb if L.algo == rm.TB else rm.random_sw
    for _ in range(n):
        now = T0 + rnd.randrange(0, 10 * L.w)
        p = rnd.randrange(1, L.max + 2)                 # max + 1: NEVER
        s = gen(rnd, L, min(p, L.max), now)
        got, want = rm.search(L, p, now, s, stats), _oracle_scan(L, p, now, s)
        if got != want:
            bad.append((p, now, s, got, want))
    assert not bad, (name, len(bad), bad[:3])
    se, bi = stats.get("searches", 0), stats.get("bisections", 0)
    print(f"{name}: {n} states, {se} searched, {bi} fell back to bisection "
          f"({100.0 * bi / max(1, se):.2f}% of the searches)")
    assert se >= n // 20, (name, "too few states needed a search", se)
    assert bi < 0.05 * se, (name, bi, se)
    return se, bi


# small windows keep the full scan short; the arithmetic classes do not depend on the size
TB_CASES = [
    ("tb 5 @ 100/s w 30", (rm.TB, 5, 30, 100.0), 7000),
    ("tb 5 @ 2/s w 20 (expiry at last + 2w + 1 before refill)", (rm.TB, 5, 20, 2.0), 7000),
    ("tb 7 @ 33.3/s w 25", (rm.TB, 7, 25, 33.3), 7000),
]
# the window fraction's classes (rl_device.hpp kLfPctMul / kLfPctFma / divide): 25 and 59 are
# one-multiply windows, 24 and 50 need the fma correction; the divide class starts beyond the
# 2^22 ms the engine checks by exhaustion, so it is forced on a small window here (the same
# arithmetic: one IEEE division)
SW_CASES = [
    ("sw 10 / 25 ms (mul)", (rm.SW, 10, 25), {}, rm.LF_MUL, 4000),
    ("sw 6 / 59 ms (mul)", (rm.SW, 6, 59), {}, rm.LF_MUL, 2000),
    ("sw 10 / 24 ms (fma)", (rm.SW, 10, 24), {}, rm.LF_FMA, 4000),
    ("sw 3 / 50 ms (fma)", (rm.SW, 3, 50), {}, rm.LF_FMA, 2000),
    ("sw 10 / 37 ms (divide)", (rm.SW, 10, 37), {"lflags": 0}, 0, 4000),
    ("sw 10 / 40 ms, cache ttl 10", (rm.SW, 10, 40, 0.0, 10), {}, rm.LF_FMA, 4000),
    ("sw 4 / 16 ms, cache ttl 30", (rm.SW, 4, 16, 0.0, 30), {}, rm.LF_MUL, 2000),
]


def test_token_bucket_search_equals_the_oracle_scan():
    assert sum(c[2] for c in TB_CASES) >= 20000
    for i, (name, spec, n) in enumerate(TB_CASES):
        _run(name, rm.Lim(*spec), n, 100 + i)


def test_sliding_window_search_equals_the_oracle_scan():
    assert sum(c[4] for c in SW_CASES) >= 20000
    for i, (name, spec, kw, flags, n) in enumerate(SW_CASES):
        L = rm.Lim(*spec, **kw)
        assert L.lflags == flags, (name, L.lflags)
        _run(name, L, n, 200 + i)


def test_never_invalid_and_absent():
    L = rm.Lim(rm.TB, 5, 1000, 10.0)
    s = {"tokens": 0.0, "last": T0, "exists": True}
    assert rm.search(L, 6, T0, s) == rm.NEVER
    assert rm.search(L, 0, T0, s) == rm.INVALID and rm.search(L, -3, T0, s) == rm.INVALID
    assert rm.search(L, 1, T0, s) == 100 and rm.search(L, 3, T0 + 50, s) == 250
    assert rm.search(L, 5, T0, dict(s, exists=False)) == 0
    assert rm.search(L, 5, T0 + 2001, s) == 0                     # the hash expired
    S = rm.Lim(rm.SW, 10, 200)
    assert rm.search(S, 11, T0, {"b1_start": T0, "b1_cnt": 0, "b1_off": 0, "b0_cnt": 0,
                                 "b0_off": 0, "x": 0}) == rm.NEVER
    full = {"b1_start": T0, "b1_cnt": 10, "b1_off": 20, "b0_cnt": 0, "b0_off": 0, "x": 0}
    # 10 in the current bucket: the next window weighs them down ms by ms
    assert rm.search(S, 1, T0 + 30, full) == rm.scan(S, 1, T0 + 30, full) > 170
    assert rm.search(S, 10, T0 + 30, full) == 20 + 200 + 1 - 30  # the bucket's PEXPIRE lapses


@pytest.mark.parametrize("seed", [1, 2])
def test_bound(seed):
    """wait <= 2 * window + cache ttl + 1 on every state."""
    rnd = random.Random(seed)
    for L in (rm.Lim(rm.TB, 5, 300, 0.5), rm.Lim(rm.SW, 10, 200, 0.0, 50)):
        gen = rm.random_tb if L.algo == rm.TB else rm.random_sw
        for _ in range(3000):
            now = T0 + rnd.randrange(0, 10 * L.w)
            p = rnd.randrange(1, L.max + 1)
            w = rm.search(L, p, now, gen(rnd, L, p, now))
            assert 0 <= w <= 2 * L.w + L.cache_ttl + 1


def test_bisection_fallback_is_exact(monkeypatch):
    """With the guesses disabled every search ends in the bisection: same answers."""
    monkeypatch.setattr(rm, "sw_guess_window", lambda W, lo, prev, curr, room, w: -1)
    rnd = random.Random(7)
    for L in (rm.Lim(rm.TB, 5, 30, 100.0), rm.Lim(rm.SW, 10, 25), rm.Lim(rm.SW, 10, 40, 0.0, 10)):
        L.inv_rate = 0.0                                 # the token-bucket guess becomes `last`
        gen = rm.random_tb if L.algo == rm.TB else rm.random_sw
        stats = {}
        for _ in range(1500):
            now = T0 + rnd.randrange(0, 10 * L.w)
            p = rnd.randrange(1, L.max + 1)
            s = gen(rnd, L, p, now)
            assert rm.search(L, p, now, s, stats) == _oracle_scan(L, p, now, s), (p, now, s)
        assert stats.get("bisections", 0) > 50, stats
