"""The small-batch path (rl_tune "small_batch", DESIGN.md §4 "Small batches"): one kernel launch of
one workgroup decides a batch of up to RL_SMALL_BATCH_MAX requests. Every case runs the same
stream on an engine with the path on, on a twin with it off and on the C oracle (small_cases.Pair)
and asserts, bit for bit, allowed / remaining / tokens_after, the returned status and
rl_last_status, and every rl_batch_stats field except the two that describe the pipeline's own
work (small_cases.PATH_FIELDS: routed, hot_regions), then the exact taken / declined counts.
Device outputs carry sentinel guard words past n. Shapes: the wave and round boundaries of the
512-thread workgroup (63..65, 255..257, 511..513 are inside MAX - 1 / MAX's rounds), one region
and many, more regions than waves."""
import numpy as np
import pytest

import rl_amd
import small_cases as sc
from small_cases import MAX, NS, T0, Pair

pytestmark = pytest.mark.gpu

CACHE_SW = (rl_amd.SW, 3, 1000, 0.0, 0, 200)          # local cache, 200 ms


def test_tune_key_and_default():
    P = Pair([sc.SW, sc.TB], small=None)
    rng = np.random.default_rng(3)
    for n in (1, 64, MAX, MAX + 1):
        P.host(*sc.mixed_batch(rng, n, 50, T0))
        P.expect()                                      # key untouched: nothing taken, nothing declined
    with pytest.raises(rl_amd.RlError):
        P.on.tune("small_batch", -1)
    P.on.tune("small_batch", 0)
    P.host(*sc.mixed_batch(rng, 5, 50, T0 + 50))
    P.expect()
    P.on.tune("small_batch", 8)                         # n <= min(v, MAX) takes it; above v: not counted
    P.host(*sc.mixed_batch(rng, 8, 50, T0 + 60))
    P.expect(taken=1)
    P.host(*sc.mixed_batch(rng, 9, 50, T0 + 70))
    P.expect()
    P.close()


def test_sizes_host():
    sc.run_sizes()


def test_sizes_device():
    sc.run_sizes(device=True)


@pytest.mark.parametrize("lim", [0, 1], ids=["sw", "tb"])
def test_one_key_repeated_at_its_limit(lim):
    P = Pair([sc.SW, sc.TB])
    rng = np.random.default_rng(4)
    allowed = total = 0
    for n, t in ((300, T0), (MAX, T0 + 400), (65, T0 + 1300)):
        keys = np.full(n, 42, np.uint64)
        permits = rng.integers(1, 5, size=n, dtype=np.int32)
        now = (t + np.arange(n) // 4).astype(np.int64) * NS
        a, r, tk, st = P.host(keys, permits, now, np.full(n, lim, np.uint16))
        allowed, total = allowed + int(a.sum()), total + n
        P.expect(taken=1)
    assert 0 < allowed < total
    P.close()


def test_all_keys_distinct():
    P = Pair([sc.SW, sc.TB])
    keys = np.arange(1, MAX + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    now = np.full(MAX, T0 * NS, np.int64)
    a, r, tk, st = P.host(keys, np.ones(MAX, np.int32), now, (np.arange(MAX) % 2).astype(np.uint16))
    assert a.all() and P.on.stats()["distinct_keys"] == MAX
    P.expect(taken=1)
    P.device(keys[:700], np.ones(700, np.int32), now[:700] + 10 * NS, (np.arange(700) % 2).astype(np.uint16))
    P.expect(taken=1)
    P.close()


def test_one_region_overflows_on_a_fixed_table():
    sc.run_one_region(fixed=True)


def test_one_region_grows_the_table():
    sc.run_one_region(fixed=False)


def test_limiters_with_a_local_cache():
    P = Pair([sc.SW, sc.TB, CACHE_SW])
    rng = np.random.default_rng(6)
    # deny, then ask again within the cache's TTL (a cache hit), then after it
    n = 12
    keys = np.repeat(np.array([7, 8], np.uint64), n // 2)
    lim = np.full(n, 2, np.uint16)
    for dt in (0, 50, 120, 400):
        a, r, tk, st = P.host(keys, np.ones(n, np.int32), np.full(n, (T0 + dt) * NS, np.int64), lim)
        P.expect(taken=1)
    assert P.oracle.cache_hits() > 0
    for i in range(4):                                   # all three limiters in one batch
        k, p, now, l = sc.mixed_batch(rng, 257, 40, T0 + 500 + 90 * i, n_lim=3)
        P.host(k, p, now, l)
        P.expect(taken=1)
    P.close()


def test_wide_results_are_declined():
    """max_permits above what the 16-byte record holds: 32-byte records, the pipeline's."""
    P = Pair([(rl_amd.SW, 5_000_000, 1000, 0.0), sc.TB])
    rng = np.random.default_rng(7)
    k, p, now, l = sc.mixed_batch(rng, 65, 20, T0, span_ms=1)
    p[3] = 4_500_000
    P.host(k, p, now, l)
    P.expect(declined=1)
    P.device(k, p, now + 7 * NS, l)
    P.expect(declined=1)
    P.close()


def test_operations_interleaved():
    P = Pair([sc.SW, sc.TB])
    rng = np.random.default_rng(8)
    for i, n in enumerate((1, 64, 300, MAX)):
        k, p, now, l = sc.mixed_batch(rng, n, 9, T0 + 100 * i)
        ops = rng.choice(np.array([rl_amd.OP_ACQUIRE, rl_amd.OP_PEEK, rl_amd.OP_RESET], np.uint8), size=n,
                         p=[0.6, 0.25, 0.15])
        P.host(k, p, now, l, ops)
        P.expect(taken=1)
        P.device(k, p, now + 45 * NS, l, ops)
        P.expect(taken=1)
    P.close()


def test_invalid_requests():
    P = Pair([sc.SW, sc.TB])
    rng = np.random.default_rng(10)
    n = 130
    k, p, now, l = sc.mixed_batch(rng, n, 30, T0)
    p[::7] = 0
    p[3::11] = -5
    l[5::13] = 9                                         # unknown limiter
    now[5::13] = -(1 << 62)                              # an invalid request's time is never read
    ops = np.zeros(n, np.uint8)
    ops[::17] = 3                                        # unknown operation
    a, r, tk, st = P.host(k, p, now, l, ops)
    assert st == rl_amd.RL_E_INVALID_REQUEST and (r[::7] == sc.REM_INVALID).all()
    P.expect(taken=1)
    # an all-invalid batch
    a, r, tk, st = P.host(k[:70], np.zeros(70, np.int32), now[:70] + 50 * NS, None, None)
    assert st == rl_amd.RL_E_INVALID_REQUEST and (r == sc.REM_INVALID).all() and not a.any()
    P.expect(taken=1)
    a, r, tk, st = P.device(k[:1], np.zeros(1, np.int32), now[:1] + 60 * NS, None, None)
    P.expect(taken=1)
    P.close()


def test_null_arrays():
    P = Pair([sc.SW, sc.TB])
    rng = np.random.default_rng(11)
    k, p, now, l = sc.mixed_batch(rng, 200, 30, T0, span_ms=1)
    P.host(k, p, now, None, None)                        # limiter and op null: limiter 0, acquires
    P.expect(taken=1)
    P.host(k, p, now + NS, l, None, want_tokens=False)   # tokens_after null
    P.expect(taken=1)
    P.device(k, p, now + 2 * NS, None, None, want_tokens=False)
    P.expect(taken=1)
    P.device(k, p, now + 3 * NS, l, None)
    P.expect(taken=1)
    P.close()


def test_engine_with_no_limiters():
    P = Pair([], oracle=False)
    k = np.arange(1, 6, dtype=np.uint64)
    a, r, tk, st = P.host(k, np.ones(5, np.int32), np.full(5, T0 * NS, np.int64))
    assert st == rl_amd.RL_E_INVALID_REQUEST and (r == sc.REM_INVALID).all()
    P.expect(declined=1)
    P.device(k, np.ones(5, np.int32), np.full(5, T0 * NS, np.int64))
    P.expect(declined=1)
    P.close()


def test_span_beyond_the_compact_record():
    P = Pair([sc.SW, sc.TB])
    n = 66
    k = np.arange(1, n + 1, dtype=np.uint64)
    now = np.full(n, T0 * NS, np.int64)
    now[n // 2:] += ((1 << 32) + 5) * NS
    l = (np.arange(n) % 2).astype(np.uint16)
    # host form: rejected untouched by the small kernel, decided in 32-byte records by the pipeline
    a, r, tk, st = P.host(k, np.ones(n, np.int32), now, l)
    assert st == rl_amd.RL_OK and a.all()
    P.expect(taken=1, declined=1)
    # device form: rejected, as on the twin
    a, r, tk, st = P.device(k, np.ones(n, np.int32), now + NS, l, oracle=False)
    assert st == rl_amd.RL_E_INVALID_ARG and (r == sc.REM_INVALID).all() and not a.any()
    P.expect(taken=1)
    # and the state is what the host batch left
    P.host(k, np.ones(n, np.int32), now + 2 * NS, l, want_tokens=True, oracle=False)
    P.expect(taken=1, declined=1)
    P.close()


def test_a_batch_earlier_than_the_last_under_skew():
    P = Pair([sc.SW, sc.TB], max_skew_ms=500)
    rng = np.random.default_rng(12)
    k, p, now, l = sc.mixed_batch(rng, 300, 25, T0 + 600)
    P.host(k, p, now, l)
    P.expect(taken=1)
    l2 = np.zeros(300, np.uint16)                        # (sliding window, same window: the oracle agrees)
    P.host(k, p, now - 250 * NS, l2)
    P.expect(taken=1)
    P.host(k, p, now + 30 * NS, l)
    P.expect(taken=1)
    P.close()


def test_rollover_and_expiry_between_batches():
    P = Pair([sc.SW, sc.TB])
    rng = np.random.default_rng(13)
    for dt in (0, 700, 1100, 1900, 2100, 9000, 9001):   # same window, next window, both TTLs run out
        k, p, now, l = sc.mixed_batch(rng, 257, 12, T0 + dt, span_ms=1)
        P.host(k, p, now, l)
        P.expect(taken=1)
    P.digests_equal((T0 + 9002) * NS)
    P.close()


def test_interleaving_with_the_pipeline():
    sc.run_interleaving()


def test_entry_points():
    import torch
    P = Pair([sc.SW, sc.TB])
    rng = np.random.default_rng(14)
    k, p, now, l = sc.mixed_batch(rng, 129, 20, T0, span_ms=1)
    P.device(k, p, now, l)                               # the engine's stream
    P.expect(taken=1)
    P.device(k, p, now + NS, l, stream=torch.cuda.Stream())   # a caller's stream
    P.expect(taken=1)
    P.host(k, p, now + 2 * NS, l)                        # pageable buffers
    P.expect(taken=1)
    for e in (P.on, P.off):
        for arr in (k, p, now, l):
            assert e.pin_host(arr) == rl_amd.RL_OK
    P.host(k, p, now + 3 * NS, l)                        # rl_pin_host-ed buffers
    P.expect(taken=1)
    for e in (P.on, P.off):
        for arr in (k, p, now, l):
            e.unpin_host(arr)
    # rl_available and rl_reset are batches of this size too
    q = np.unique(k)
    tq = np.full(len(q), (T0 + 5) * NS, np.int64)
    for lim in (0, 1):
        av_on, st_on = P.on.available(lim, q, tq)
        av_off, st_off = P.off.available(lim, q, tq)
        _, orem, _, _ = P.oracle.run(q, np.ones(len(q), np.int32), tq, np.full(len(q), lim, np.uint16),
                                     np.full(len(q), rl_amd.OP_PEEK, np.uint8))
        assert sc.same(av_on, av_off) and sc.same(av_on, orem) and st_on == st_off == rl_amd.RL_OK
        P.expect(taken=1)
        assert P.on.reset(lim, q[::2], tq[::2]) == P.off.reset(lim, q[::2], tq[::2]) == rl_amd.RL_OK
        P.oracle.run(q[::2], np.ones(len(q[::2]), np.int32), tq[::2], np.full(len(q[::2]), lim, np.uint16),
                     np.full(len(q[::2]), rl_amd.OP_RESET, np.uint8))
        P.expect(taken=1)
    P.host(k, p, now + 9 * NS, l)
    P.expect(taken=1)
    P.close()


def test_pipelined_engine_declines():
    """RL_OPT_PIPELINE: a small batch right behind a pipelined batch on the same keys is declined
    (never reordered): it follows the batch in flight through the pipeline."""
    P = Pair([sc.SW, sc.TB], small=MAX, pipeline=True, max_batch=1 << 14)
    rng = np.random.default_rng(15)
    k, p, now, l = sc.mixed_batch(rng, 6000, 40, T0)
    P.device(k, p, now, l)
    P.expect()
    P.device(k[:50], p[:50], now[:50] + 45 * NS, l[:50])
    P.expect(declined=1)
    P.host(k[:9], p[:9], now[:9] + 50 * NS, l[:9])
    P.expect(declined=1)
    P.close()


def test_stage_timing_and_string_keys_decline():
    P = Pair([sc.SW, sc.TB], small=MAX, stage_timing=True)
    rng = np.random.default_rng(16)
    k, p, now, l = sc.mixed_batch(rng, 40, 10, T0)
    P.host(k, p, now, l)
    P.expect(declined=1)
    P.close()
    P = Pair([sc.SW, sc.TB], small=MAX, oracle=False)
    blob, off = rl_amd.pack_keys([f"user:{i % 5}" for i in range(20)])
    res = [e.execute_batch_keys(blob, off, np.ones(20, np.int32), np.full(20, T0 * NS, np.int64))
           for e in (P.on, P.off)]
    assert sc.same(res[0][0], res[1][0]) and sc.same(res[0][1], res[1][1])
    P.expect(declined=1)
    P.close()
