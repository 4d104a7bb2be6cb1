#!/usr/bin/env python3
"""CPU model of the per-query work of the quota lookup (csrc/rl_quota.hip `k_quota`) for ONE
query on a key's state: the peek at now, the reset search and the retry search. The exact
predicates and the search itself are those of tools/retry_after_model.py (the model of
csrc/rl_retry.hpp `retry_search`, which both kernels run): the reset search is that search in
its `full` mode, whose predicate is "the peek at t reads max", with the cache word ignored.

`reset_scan` is the definition, min{t >= now : A(t) == max} - now, by a full scan that assumes
no monotonicity. `main` compares the two on random states, and both with the retry search of
p = max on the same limiter without its local cache (the identity of DESIGN.md §4 "Quota
queries"): a guess that is off, a bound that is short or a loop that does not end shows up here
instead of on the GPU (tests/test_quota_model.py checks the model against the oracle). Test tooling only:
nothing in the product imports it.

usage: tools/quota_model.py [--n N] [--seed S]
"""
import argparse
import importlib.util
import os
import random

_spec = importlib.util.spec_from_file_location(
    "retry_after_model", os.path.join(os.path.dirname(os.path.abspath(__file__)), "retry_after_model.py"))
rm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rm)

SW, TB = rm.SW, rm.TB
NEVER, INVALID = rm.NEVER, -2          # RL_RETRY_NEVER, RL_QUOTA_INVALID
Lim = rm.Lim

ZERO_TB = {"tokens": 0.0, "last": 0, "exists": False}
ZERO_SW = {"b1_start": 0, "b1_cnt": 0, "b1_off": 0, "b0_cnt": 0, "b0_off": 0, "x": 0}


def without_cache(L):
    """L with its local cache off (the same arithmetic otherwise)."""
    return Lim(L.algo, L.max, L.w, L.refill_per_s, 0, L.lflags)


def query(L, now, s, p=None, skip=False, stats=None):
    """k_quota's answers for one valid query: (remaining, reset_ms, retry_ms or None). `s` is the
    key's slot state, or None for a key without a slot (all zero words)."""
    if p is not None and not skip and p <= 0:
        return INVALID, INVALID, INVALID
    have = s is not None
    if not have:
        s = ZERO_TB if L.algo == TB else ZERO_SW
    rem = rm.peek(L, now, s)
    reset = 0
    if have and rem != L.max:
        reset = rm.search(L, L.max, now, s, stats, full=True)
    retry = None
    if p is not None:
        retry = 0
        if not skip:
            if p > L.max:
                retry = NEVER
            elif have:
                retry = rm.search(L, p, now, s)
    return rem, reset, retry


def reset_scan(L, now, s):
    """The definition: the first t in now .. now + 2w + 2 at which the peek reads max, by a full
    scan (no monotonicity used; it asserts that A never drops after first reaching max)."""
    first = None
    for t in range(now, now + 2 * L.w + 2 + 1):
        ok = rm.peek(L, t, s) == L.max
        if ok and first is None:
            first = t
        assert ok or first is None, ("A drops after reaching max", L.algo, now, t, s)
    assert first is not None, ("no full quota inside the bound", L.algo, now, s)
    return first - now


def random_state(rnd, L, now):
    """retry_after_model's random states, aimed at the full quota (p = max): token balances
    within 1 ulp of cap, window estimates at 0 and 1."""
    gen = rm.random_tb if L.algo == TB else rm.random_sw
    return gen(rnd, L, L.max, now)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rnd = random.Random(a.seed)
    t0 = 1_700_000_000_000
    lims = [("tb 5 @ 10/s w 1000", Lim(TB, 5, 1000, 10.0)), ("tb 5 @ 0.5/s w 300", Lim(TB, 5, 300, 0.5)),
            ("tb 7 @ 3.3/s w 1000", Lim(TB, 7, 1000, 3.3)), ("sw 10 / 200 ms", Lim(SW, 10, 200)),
            ("sw 10 / 200 ms, cache 50", Lim(SW, 10, 200, 0.0, 50)), ("sw 3 / 1000 ms", Lim(SW, 3, 1000))]
    for name, L in lims:
        stats, bad, ident, pos = {}, 0, 0, 0
        N = without_cache(L)
        for _ in range(a.n):
            now = t0 + rnd.randrange(0, 10 * L.w)
            s = random_state(rnd, L, now)
            rem, reset, _ = query(L, now, s, stats=stats)
            bad += reset != reset_scan(L, now, s) or rem != rm.peek(L, now, s)
            ident += reset != rm.search(N, L.max, now, dict(s, x=0) if L.algo == SW else s)
            pos += reset > 0
        se, bi = stats.get("searches", 0), stats.get("bisections", 0)
        print(f"{name}: {a.n} queries, {pos} with reset > 0, {se} searched, {bi} bisected "
              f"({100.0 * bi / max(1, se):.2f}% of the searches), {bad} mismatches with the scan, "
              f"{ident} with the retry search of p = max")


if __name__ == "__main__":
    main()
