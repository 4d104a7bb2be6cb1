"""Packed result widths and compact-record limits at their edge values, through every kernel
that writes a result (region, hot chain / fill, solo, fill_invalid) and every unpermute variant.

res_bytes_for (rl_device.hpp) switches u8 / u16 / u32 / u64 at max_permits 124|125, 32764|32765
and 4194302|4194303 (kCompactMaxPermits). Per edge value m, a sliding-window and a token-bucket
limiter of max m get a request set that produces the top remaining of the width (m, from a peek
of an absent key), m - 1, 1 and 0, the status values -1 (token bucket, permits > max) and -2
(invalid) beside token-bucket balances of exactly -1, -2, -3 (the lowest packed value), -4 (the
first through the escape code kResEscape), -1000 and one below -2^31 (time regression: at 1000
tokens/s the balance falls by one per ms), and acquires of 4194302, 4194303, 4194304 and
2^31 - 1 permits (the compact record clamps at kPermitMask). Everything is compared with the CPU
oracle bit for bit, balances included, and the oracle's output is asserted to contain each
targeted value (tests/test_result_widths_model.py, on the CPU)."""
import functools

import numpy as np
import pytest

import rl_amd
from oracle.coracle import COracle
from test_gpu_parity import NS, T0, assert_same

pytestmark = pytest.mark.gpu

WIDTHS = {124: 1, 125: 2, 32_764: 2, 32_765: 4, 4_194_302: 4, 4_194_303: 8}
W_MS = 60_000
BIG = (4_194_302, 4_194_303, 4_194_304, (1 << 31) - 1)
REGRESS = (1, 2, 3, 4, 1000)
DEEP = (1 << 31) + 5                              # ms of regression: a balance below -2^31
A, PEEK = rl_amd.OP_ACQUIRE, rl_amd.OP_PEEK


def lims_for(m, cache_ttl=0):
    sw = [rl_amd.SW, m, W_MS, 0.0] + ([0, cache_ttl] if cache_ttl else [])
    return [sw, [rl_amd.TB, m, W_MS, 1000.0]]


def key(i):
    return int(rl_amd.mix64(np.array([i], np.uint64) + np.uint64(0xE1 << 40))[0])


@functools.lru_cache(maxsize=None)
def request_set(m):
    """(trace, n_main): ~4K requests within 3 s in arrival order, then a tail of token-bucket
    requests 2^31 + 5 ms in the past (a batch of their own: a compact record holds +-2^31 ms
    around its batch's first request)."""
    rng = np.random.default_rng(m)
    rows = []                                      # (order, key, permits, ms, limiter, op)
    t0 = T0 + 2000

    def add(order, k, p, ms, lim, op=A):
        rows.append((order, k, p, ms, lim, op))

    nk = 0
    for lim in (0, 1):
        for j in range(8):                          # m (peek of an absent key), m - 1, denial at m + 1
            add(10 + j, key(nk), 1, t0 + j, lim, PEEK)
            add(20 + j, key(nk), 1, t0 + 10 + j, lim)
            add(30 + j, key(nk), m + 1, t0 + 20 + j, lim)
            nk += 1
        for p in BIG:                               # fresh keys: only permits <= max are allowed
            add(40, key(nk), p, t0 + 40, lim)
            add(41, key(nk), 1, t0 + 41, lim, PEEK)
            nk += 1
    for j in range(4):                              # token bucket: m - 1 taken -> 1, then -> 0
        add(50, key(nk), m - 1, t0 + 50, 1)
        add(51, key(nk), 1, t0 + 50, 1)
        add(52, key(nk), 1, t0 + 50, 1, PEEK)
        nk += 1
    drain_at = t0 + 2500
    x_keys = [key(nk + j) for j in range(4)]
    nk += 4
    for j, k in enumerate(x_keys):                  # drained, then requests from the past
        add(2500, k, m, drain_at, 1)
        for d in REGRESS:
            add(2600 + 10 * j, k, 1, drain_at - d, 1)
            add(2601 + 10 * j, k, 1, drain_at - d, 1, PEEK)
    for i, (p, lim, op) in enumerate(((0, 0, A), (-7, 1, A), (1, 7, A), (1, 0, 9), (1, 255, PEEK))):
        for j in range(6):                          # invalid: permits, limiter id, op
            add(100 + 400 * j + i, key(nk), p, t0 + 100 + 400 * j, lim, op)
        nk += 1
    hot = (key(nk), key(nk + 1))                    # one hot key per limiter, at its limit for small m
    nk += 2
    for lim in (0, 1):
        for j in range(700):
            add(200 + 3 * j, hot[lim], 1 + (j % 7 == 0), t0 + 200 + 3 * j, lim, PEEK if j % 50 == 49 else A)
    n_bg = 2500
    ranks = rng.integers(0, 700, n_bg)
    ms = np.sort(rng.integers(0, 3000, n_bg))
    for j in range(n_bg):
        add(int(ms[j]), key(10_000 + int(ranks[j])), int(rng.integers(1, 4)), t0 + int(ms[j]),
            int(ranks[j] % 2), PEEK if rng.random() < 0.05 else A)
    rows.sort(key=lambda r: r[0])
    n_main = len(rows)
    for j, k in enumerate(x_keys):                  # the tail
        rows.append((0, k, 1, drain_at - DEEP - j, 1, A))
        rows.append((0, k, 1, drain_at - DEEP - j, 1, PEEK))
    for j in range(20):                             # (fresh token buckets beside them)
        rows.append((0, key(20_000 + j), 2, drain_at - DEEP - 4, 1, A))
    tr = (np.array([r[1] for r in rows], np.uint64), np.array([r[2] for r in rows], np.int32),
          np.array([r[3] for r in rows], np.int64) * NS, np.array([r[4] for r in rows], np.uint16),
          np.array([r[5] for r in rows], np.uint8))
    for a in tr:
        a.setflags(write=False)
    return tr, n_main


@functools.lru_cache(maxsize=None)
def reference_and_hits(m, cache_ttl=0):
    """The oracle's answer to request_set(m) (read-only) and its local-cache hits."""
    tr, _ = request_set(m)
    o = COracle(lims_for(m, cache_ttl))
    want = o.run(*tr)[:3]
    for a in want:
        a.setflags(write=False)
    return want, o.cache_hits()


def reference(m, cache_ttl=0):
    return reference_and_hits(m, cache_ttl)[0]


def run(lims, tr, cuts, tune=None, want_tokens=True, **kw):
    kw.setdefault("max_batch", 1 << 16)
    kw.setdefault("capacity", 1 << 12)
    e = rl_amd.Engine(**kw)
    for l in lims:
        e.add_limiter(*l)
    for k, v in (tune or {}).items():
        e.tune(k, v)
    got, stats = [[], [], []], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        ga, gr, gt, st = e.execute(*(x[a:b] for x in tr), want_tokens=want_tokens)
        assert st in (rl_amd.RL_OK, rl_amd.RL_E_INVALID_REQUEST), rl_amd.strerror(st)
        got[0].append(ga); got[1].append(gr); got[2].append(gt)
        stats.append(e.stats())
    t = None if not want_tokens else np.concatenate(got[2])
    return (np.concatenate(got[0]), np.concatenate(got[1]), t), e, stats


# ---------------------------------------------------------------- widths
@pytest.mark.parametrize("m", list(WIDTHS))
def test_result_width_at_the_edges(m):
    e = rl_amd.Engine(max_batch=1 << 10, capacity=1)
    for l in lims_for(m):
        e.add_limiter(*l, capacity=1)
    assert e.result_width() == WIDTHS[m]
    e.close()


def test_result_width_is_the_widest_limiters():
    e = rl_amd.Engine(max_batch=1 << 10, capacity=1)
    e.add_limiter(rl_amd.SW, 3, 1000, 0.0, capacity=1)
    assert e.result_width() == 1
    e.add_limiter(rl_amd.TB, 125, 1000, 1.0, capacity=1)
    assert e.result_width() == 2
    e.close()


# ---------------------------------------------------------------- paths
PATHS = {
    "regions": dict(),
    "hot": dict(tune={"hot_threshold": 1}),
    "solo": dict(cache_ttl=50, tune={"solo_threshold": 64}),
    "unpermute_split0": dict(tune={"unpermute_split": 0}),
    "unpermute_split1": dict(tune={"unpermute_split": 1}),
    "two_pass": dict(capacity=1 << 22),
    "no_tokens": dict(want_tokens=False),
    "two_batches": dict(halves=True),
}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("m", list(WIDTHS))
def test_edge_values_through(m, path):
    kw = dict(PATHS[path])
    ttl = kw.pop("cache_ttl", 0)
    halves = kw.pop("halves", False)
    tr, n_main = request_set(m)
    want = reference(m, ttl)
    cuts = [0, n_main // 2, n_main, len(tr[0])] if halves else [0, n_main, len(tr[0])]
    got, e, stats = run(lims_for(m, ttl), tr, cuts, **kw)
    assert e.result_width() == WIDTHS[m]
    assert_same(got, want if kw.get("want_tokens", True) else (want[0], want[1], None), f"{path} m={m}")
    if path == "hot":
        assert all(s["hot_regions"] > 0 for s in stats), stats
    if path == "solo":
        # k_solo has no counter of its own. The cache it serves has one: the sliding window's hot
        # key is rejected from the cache once it sits at max, which 700 requests reach only for
        # m <= 125 (the oracle's own count says so), so for the larger m the row is parity alone.
        hits = reference_and_hits(m, ttl)[1]
        assert (hits > 0) == (m <= 125)
        assert sum(s["cache_hits"] for s in stats) == hits
    e.close()


# ---------------------------------------------------------------- -3 as a status beside the escape
@pytest.mark.parametrize("m", [5, 125])                              # widths 1 and 2
def test_capacity_error_beside_real_minus_three(m):
    """A one-bin fixed table that overflows (remaining -3 = REM_ERROR as a status) in the same
    batch as token-bucket balances of exactly -3 (packed, the lowest value) and -4 (escaped)."""
    lim = [rl_amd.TB, m, W_MS, 1000.0]
    e = rl_amd.Engine(max_batch=1 << 16, capacity=1)
    e.add_limiter(*lim, capacity=1)                  # MIN_REGIONS regions
    assert e.result_width() == (1 if m == 5 else 2)
    o = COracle([lim])
    xs = rl_amd.mix64(np.arange(4, dtype=np.uint64) + np.uint64(0xE2 << 40))
    t1 = (T0 + 5000) * NS
    first = (xs, np.full(4, m, np.int32), np.full(4, t1, np.int64))
    got = e.execute(*first)
    assert got[3] == rl_amd.RL_OK
    assert_same(got[:3], o.run(*first)[:3], "drain")
    n = 3000
    keys = np.concatenate([rl_amd.mix64(np.arange(n, dtype=np.uint64)), np.repeat(xs, 3)])
    now = np.concatenate([np.full(n, t1, np.int64),
                          np.tile(t1 - np.array([3, 4, 70_000], np.int64) * NS, 4)])
    order = np.random.default_rng(m).permutation(len(keys))
    keys, now = keys[order], now[order]
    ones = np.ones(len(keys), np.int32)
    a, r, t, st = e.execute(keys, ones, now)
    assert st == rl_amd.RL_E_CAPACITY
    wa, wr, wt, _ = o.run(keys, ones, now)
    is_x = np.isin(keys, xs)
    assert sorted(set(wr[is_x].tolist())) == [-70_000, -4, -3]
    err = (r == rl_amd.REM_ERROR) & ~is_x
    bits = rl_amd.MIN_REGIONS.bit_length() - 1
    region = (rl_amd.mix64(np.concatenate([rl_amd.mix64(np.arange(n, dtype=np.uint64)), xs]))
              >> np.uint64(64 - bits)).astype(np.int64)
    overflow = np.maximum(np.bincount(region, minlength=rl_amd.MIN_REGIONS) - rl_amd.REGION_SLOTS, 0).sum()
    assert overflow > 0 and err.sum() == overflow and not a[err].any()
    ok = ~err
    assert_same((a[ok], r[ok], t[ok]), (wa[ok], wr[ok], wt[ok]), f"beside the overflow m={m}")
    assert (r == -3).sum() == overflow + 4
    e.close()


# ---------------------------------------------------------------- the record's 8-bit limiter field
@pytest.mark.parametrize("hot", [0, 1])
def test_255_limiters(hot):
    lims = [[rl_amd.SW, 3 + i % 5, 1000, 0.0] if i % 2 == 0 else [rl_amd.TB, 3 + i % 5, 1000, 2.0]
            for i in range(255)]
    e = rl_amd.Engine(max_batch=1 << 14, capacity=1)
    for l in lims:
        e.add_limiter(*l, capacity=1)
    if hot:
        e.tune("hot_threshold", 1)
    assert e.result_width() == 1
    rng = np.random.default_rng(255)
    n = 6000
    lim = np.array([0, 127, 128, 254, 255], np.uint16)[rng.integers(0, 5, n)]
    keys = rl_amd.mix64(rng.integers(0, 40, n).astype(np.uint64) + np.uint64(0xE3 << 40))
    now = (T0 * NS + np.sort(rng.integers(0, 3000 * NS, n))).astype(np.int64)
    permits = rng.integers(1, 4, n).astype(np.int32)
    op = np.where(rng.random(n) < 0.05, PEEK, A).astype(np.uint8)
    o = COracle(lims)
    h = n // 2
    for sl in (slice(0, h), slice(h, n)):
        part = tuple(x[sl] for x in (keys, permits, now, lim, op))
        got = e.execute(*part)
        assert got[3] == rl_amd.RL_E_INVALID_REQUEST
        want = o.run(*part)
        assert (want[1][part[3] == 255] == -2).all() and (part[3] == 255).any()
        for lid in (0, 127, 128, 254):
            s = part[3] == lid
            assert want[0][s].any() and not want[0][s].all(), lid
        assert_same(got[:3], want[:3], f"255 limiters hot={hot}")
    e.close()
