"""rl_limiter_usage / rl_top_consumers against the oracle's Redis keyspace, bit-exact.

After the same trace the census of every limiter must equal what the oracle's keyspace
(oracle/rl_oracle.py: "rl:<key>:<W>" counters and "tb:<key>" hashes with their PEXPIRE deadlines)
and its getAvailablePermits give: live keys and Redis keys from keyspace(now), available from a
PEEK of every live key, the local cache's rejecting entries from the oracle's cache. The traces
end mid-window, so sliding-window keys hold two live buckets (redis_keys > live_keys).
"""
import ctypes

import numpy as np
import pytest

import rl_amd
from oracle.coracle import COracle
from oracle.rl_oracle import PyOracle

pytestmark = pytest.mark.gpu

NS = 1_000_000
T0 = 1_700_000_000_000
# (algo, max_permits, window_ms, refill_per_s, capacity, local_cache_ttl_ms)
LIMS = [(rl_amd.SW, 5, 1000, 0.0, 0, 0), (rl_amd.TB, 10, 1000, 5.0, 0, 0),
        (rl_amd.SW, 3, 500, 0.0, 0, 0), (rl_amd.TB, 4, 300, 20.0, 0, 0),
        (rl_amd.SW, 4, 2000, 0.0, 0, 400)]
N_KEYS = 300
SPANS = ((1, T0 + 350, T0 + 3350), (2, T0 + 3350, T0 + 6350))
END = T0 + 6350
LAGS = (0, 40, 250, 700, 2500)
FIELDS = ("live_keys", "redis_keys", "exhausted_keys", "cache_blocked", "used_permits", "hist")


def make(lims=LIMS, capacity=1 << 12, **kw):
    e = rl_amd.Engine(max_batch=1 << 18, capacity=capacity, **kw)
    o = PyOracle()
    for l in lims:
        e.add_limiter(*l)
        o.add_limiter(*l)
    return e, o


def trace(seed, t_lo, t_hi, n=25000):
    rng = np.random.default_rng(seed)
    lim = rng.integers(0, len(LIMS), n).astype(np.uint16)
    keys = (rng.integers(0, N_KEYS, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
            + lim.astype(np.uint64))
    now = np.sort(rng.integers(t_lo * NS, t_hi * NS, n)).astype(np.int64)
    permits = rng.integers(1, 4, n).astype(np.int32)
    ops = np.zeros(n, np.uint8)
    ops[rng.random(n) < 0.01] = rl_amd.OP_RESET
    return keys, permits, now, lim, ops


def run_both(e, o, tr):
    a, r, t, st = e.execute(*tr)
    wa, wr, wt = o.run(*tr)
    assert st == rl_amd.RL_OK
    np.testing.assert_array_equal(a, np.asarray(wa, np.uint8))
    np.testing.assert_array_equal(r, np.asarray(wr, np.int64))


def expected(o, lid, now_ms, lims=LIMS):
    """The census of limiter lid at now_ms from the oracle, and its (used, key) list."""
    mx, ttl = lims[lid][1], lims[lid][5]
    ks = [x for x in o.keyspace(now_ms) if x[0] == lid]
    live = sorted({x[1] for x in ks})
    n = len(live)
    avail = o.run(live, [1] * n, [now_ms * NS] * n, [lid] * n, [rl_amd.OP_PEEK] * n)[1]
    used = [mx - min(max(int(a), 0), mx) for a in avail]
    hist = [0] * rl_amd.USAGE_BINS
    for u in used:
        hist[15 if u == mx else u * 16 // mx] += 1
    blocked = sum(1 for (l, _), (v, w) in o.cache.items()
                  if l == lid and v >= mx and now_ms - w < ttl) if ttl else 0
    want = {"live_keys": n, "redis_keys": len(ks), "exhausted_keys": sum(u == mx for u in used),
            "cache_blocked": blocked, "used_permits": sum(used), "hist": hist}
    return want, sorted(zip(used, live), key=lambda x: (-x[0], x[1]))


def check_census(e, lid, now_ms, want):
    got = e.limiter_usage(lid, now_ms * NS)
    assert {f: got[f] for f in FIELDS} == want, (lid, now_ms - END)
    assert got["slots"] == e.limiter_slots(lid)
    assert got["live_keys"] <= got["used_slots"] <= got["slots"]
    assert sum(got["hist"]) == got["live_keys"]
    return got


def check_top(e, lid, now_ms, order, mx, ks=(1, 7, 64, 4096)):
    L = e._L
    for k in ks:
        for min_used in (0, 1, mx):
            m = [x for x in order if x[0] >= min_used]
            keys = np.full(k + 3, 0xABCD, np.uint64)
            used = np.full(k + 3, -77, np.int64)
            n_out, n_match = ctypes.c_size_t(99), ctypes.c_uint64(99)
            st = L.rl_top_consumers(e._h, lid, now_ms * NS, k, min_used, rl_amd._p(keys),
                                    rl_amd._p(used), ctypes.byref(n_out),
                                    ctypes.byref(n_match))
            assert st == rl_amd.RL_OK
            assert n_match.value == len(m), (lid, k, min_used)
            t = min(k, len(m))
            assert n_out.value == t
            assert [(int(u), int(h)) for u, h in zip(used[:t], keys[:t])] == m[:t], (lid, k, min_used)
            assert np.all(keys[t:] == 0xABCD) and np.all(used[t:] == -77)   # untouched
            gk, gu, gm = e.top_consumers(lid, now_ms * NS, k, min_used)
            assert (gk.tolist(), gu.tolist(), gm) == ([x[1] for x in m[:t]], [x[0] for x in m[:t]], len(m))


class State:
    def __init__(self):
        self.e, self.o = make()
        for seed, lo, hi in SPANS:
            run_both(self.e, self.o, trace(seed, lo, hi))
        self._exp = {}

    def expected(self, lid, lag):
        if (lid, lag) not in self._exp:
            self._exp[(lid, lag)] = expected(self.o, lid, END + lag)
        return self._exp[(lid, lag)]


@pytest.fixture(scope="module")
def state():
    return State()


@pytest.mark.parametrize("lag", LAGS)
def test_census_matches_the_oracle(state, lag):
    got = {}
    for lid in range(len(LIMS)):
        want, _ = state.expected(lid, lag)
        got[lid] = check_census(state.e, lid, END + lag, want)
    # the inputs keep the test from going hollow
    if lag == 0:
        assert got[0]["redis_keys"] > got[0]["live_keys"] > 200          # two live buckets per key
        assert got[4]["cache_blocked"] >= 10 and got[4]["exhausted_keys"] >= 10
        assert sum(1 for h in got[1]["hist"] if h) >= 8
    if lag == 700:
        assert got[2]["live_keys"] == 0 and got[3]["live_keys"] == 0
        assert got[0]["live_keys"] > 0
    if lag == 2500:
        for lid in range(len(LIMS)):
            assert all(got[lid][f] == 0 for f in FIELDS[:5]) and not any(got[lid]["hist"])
            assert got[lid]["used_slots"] > 0                              # tombstones


@pytest.mark.parametrize("lag", [0, 250])
def test_top_consumers_match_the_oracle(state, lag):
    for lid, l in enumerate(LIMS):
        _, order = state.expected(lid, lag)
        assert len(order) > 64 or lag                                      # cuts fall inside ties
        check_top(state.e, lid, END + lag, order, l[1])


def test_invalid_arguments_with_a_live_engine(state):
    e = state.e
    with pytest.raises(rl_amd.RlError) as x:
        e.limiter_usage(len(LIMS), END * NS)
    assert x.value.status == rl_amd.RL_E_INVALID_ARG
    for lid, k, mu in ((len(LIMS), 4, 1), (0, 0, 1), (0, rl_amd.TOP_KEYS_MAX + 1, 1), (0, 4, -1)):
        with pytest.raises(rl_amd.RlError) as x:
            e.top_consumers(lid, END * NS, k, mu)
        assert x.value.status == rl_amd.RL_E_INVALID_ARG


def test_a_tie_larger_than_the_candidate_store():
    n = 100_000
    lims = [(rl_amd.SW, 1, 60_000, 0.0, 0, 0)]
    e = rl_amd.Engine(max_batch=1 << 18, capacity=1 << 17)
    e.add_limiter(*lims[0])
    rng = np.random.default_rng(5)
    keys = np.unique(rng.integers(0, 1 << 64, n + 1000, dtype=np.uint64))
    keys = rng.permutation(keys)[:n]
    now = (T0 + 1000 + np.arange(n, dtype=np.int64) // 100) * NS
    ones = np.ones(n, np.int32)
    a, r, _, st = e.execute(keys, ones, now, np.zeros(n, np.uint16), np.zeros(n, np.uint8))
    assert st == rl_amd.RL_OK and a.all()
    at = int(now[-1]) + 1000 * NS
    co = COracle([list(lims[0][:4])])
    assert co.run(keys, ones, now)[0].all()
    avail = co.run(keys, ones, np.full(n, at, np.int64), None, np.full(n, rl_amd.OP_PEEK, np.uint8))[1]
    assert not avail.any()                                                 # every key is throttled
    assert n > rl_amd.USAGE_CANDIDATES
    got_k, got_u, n_match = e.top_consumers(0, at, 4096, 1)
    assert n_match == n
    np.testing.assert_array_equal(got_k, np.sort(keys)[:4096])
    assert (got_u == 1).all()
    u = e.limiter_usage(0, at)
    assert u["exhausted_keys"] == u["live_keys"] == n and u["hist"][15] == n
    assert u["used_permits"] == n and u["redis_keys"] == n and u["slots"] == e.limiter_slots(0)
    # k = 1: the smallest key hash of the tie
    assert e.top_consumers(0, at, 1, 1)[0].tolist() == [int(keys.min())]


def test_a_tie_that_fills_one_digit_takes_a_second_pass():
    """max_permits = 5000 has 13 significant bits, so the select's first 12-bit digit is `used`
    alone: 100,000 keys with the same `used` share one bin (> RL_USAGE_CANDIDATES) and the
    refinement goes on into the key hash."""
    n, mx = 100_000, 5000
    lim = (rl_amd.TB, mx, 60_000, 1.0, 0, 0)
    e = rl_amd.Engine(max_batch=1 << 18, capacity=1 << 17)
    e.add_limiter(*lim)
    rng = np.random.default_rng(6)
    keys = rng.permutation(np.unique(rng.integers(0, 1 << 64, n + 1000, dtype=np.uint64)))[:n]
    now = np.full(n, (T0 + 1000) * NS, np.int64)
    permits = np.full(n, mx - 7, np.int32)
    permits[:10] = mx                                     # ten keys above the tie
    a, r, _, st = e.execute(keys, permits, now, np.zeros(n, np.uint16), np.zeros(n, np.uint8))
    assert st == rl_amd.RL_OK and a.all()
    at = (T0 + 3000) * NS                                 # 2 s later: two tokens are back
    co = COracle([list(lim[:4])])
    assert co.run(keys, permits, now)[0].all()
    avail = co.run(keys, permits, np.full(n, at, np.int64), None, np.full(n, rl_amd.OP_PEEK, np.uint8))[1]
    used = mx - np.clip(avail, 0, mx)
    assert set(used.tolist()) == {mx - 2, mx - 9}
    order = np.lexsort((keys, -used))
    got_k, got_u, n_match = e.top_consumers(0, at, 4096, 1)
    assert n_match == n
    np.testing.assert_array_equal(got_k, keys[order][:4096])
    np.testing.assert_array_equal(got_u, used[order][:4096])
    passes = ctypes.c_uint32(0)
    assert e._L.rl_debug_fetch(e._h, b"usage_passes", ctypes.byref(passes), 4) == 1
    assert passes.value == 3                              # two digits and the compaction
    assert (got_u[:10] == mx - 2).all() and (got_u[10:] == mx - 9).all()
    # min_used leaves only the ten keys above the tie
    got_k, got_u, n_match = e.top_consumers(0, at, 4096, mx - 2)
    assert n_match == 10 and got_k.tolist() == sorted(keys[:10].tolist()) and (got_u == mx - 2).all()
    u = e.limiter_usage(0, at)
    assert u["live_keys"] == n and u["exhausted_keys"] == 0 and u["used_permits"] == int(used.sum())
    assert u["hist"][15] == n                             # (mx - 2) * 16 // mx


@pytest.mark.parametrize("pipeline", [False, True])
def test_the_calls_only_read_and_run_behind_the_batches(pipeline):
    import torch
    e, o = make(pipeline=pipeline)
    run_both(e, o, trace(*SPANS[0]))
    now_ms = SPANS[0][2]
    before = (e.stats(), e.last_status(), e.export_state(now_ms * NS).tobytes())
    for lid, l in enumerate(LIMS):
        want, order = expected(o, lid, now_ms)
        check_census(e, lid, now_ms, want)
        check_top(e, lid, now_ms, order, l[1], ks=(7,))
    assert (e.stats(), e.last_status(), e.export_state(now_ms * NS).tobytes()) == before
    # the next segment as a device batch, not waited for: the census runs behind it
    tr = trace(*SPANS[1])
    n = tr[0].shape[0]
    dev = [torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else
                            x.view(np.int16) if x.dtype == np.uint16 else x).cuda() for x in tr]
    allowed = torch.zeros(n, dtype=torch.uint8, device="cuda")
    remaining = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.execute_device(n, *dev, allowed, remaining)
    got = [e.limiter_usage(lid, END * NS) for lid in range(len(LIMS))]
    assert e.last_status() == rl_amd.RL_OK
    wa, wr, _ = o.run(*tr)
    np.testing.assert_array_equal(allowed.cpu().numpy(), np.asarray(wa, np.uint8))
    np.testing.assert_array_equal(remaining.cpu().numpy(), np.asarray(wr, np.int64))
    for lid in range(len(LIMS)):
        want, _ = expected(o, lid, END)
        assert {f: got[lid][f] for f in FIELDS} == want


def test_a_grown_table_reports_the_same():
    e, o = make()
    for seed, lo, hi in SPANS:
        run_both(e, o, trace(seed, lo, hi))
    for lid, l in enumerate(LIMS):
        want, order = expected(o, lid, END)
        slots = e.limiter_slots(lid)
        e.grow_limiter(lid, 2 * slots)                    # load <= 0.5: at least 4 x the slots
        assert e.limiter_slots(lid) >= 4 * slots
        check_census(e, lid, END, want)
        check_top(e, lid, END, order, l[1], ks=(7, 4096))


def test_after_a_sweep_every_used_slot_is_a_live_key():
    e, o = make()
    for seed, lo, hi in SPANS:
        run_both(e, o, trace(seed, lo, hi))
    now_ms = END + 250
    tomb = sum(u["used_slots"] - u["live_keys"]
               for u in (e.limiter_usage(lid, now_ms * NS) for lid in range(4)))
    assert tomb > 0                                       # keys that expired or were reset
    e.sweep_expired(now_ms * NS)
    for lid in range(4):                                  # (limiter 4 keeps its cache entries)
        want, _ = expected(o, lid, now_ms)
        got = check_census(e, lid, now_ms, want)
        assert got["used_slots"] == got["live_keys"]


def test_edge_inputs():
    lims = [(rl_amd.SW, 2, 1000, 0.0, 0, 0), (rl_amd.TB, 2, 1000, 1.0, 0, 0)]
    e, o = make(lims)
    for lid in range(2):                                  # an empty limiter
        u = e.limiter_usage(lid, T0 * NS)
        assert u["slots"] == e.limiter_slots(lid) > 0
        assert all(u[f] == 0 for f in FIELDS[:5]) and u["used_slots"] == 0 and not any(u["hist"])
        gk, gu, gm = e.top_consumers(lid, T0 * NS, 4, 0)
        assert (len(gk), len(gu), gm) == (0, 0, 0)
    top = (1 << 64) - 1
    # 0 and ~0 exhausted, 5 and 9 not (a sliding-window acquire INCRs by one whatever it asks for)
    keys = np.array([0, top, 5, 0, top, 0, top, 9], np.uint64)
    lim = np.array([0, 0, 0, 0, 0, 1, 1, 1], np.uint16)
    permits = np.array([1, 1, 1, 1, 1, 2, 2, 1], np.int32)
    now = np.full(8, (T0 + 10) * NS, np.int64)
    run_both(e, o, (keys, permits, now, lim, np.zeros(8, np.uint8)))
    for lid in range(2):
        want, order = expected(o, lid, T0 + 10, lims)
        assert order[0] == (2, 0) and order[1] == (2, top)            # first and last of the tie
        got = check_census(e, lid, T0 + 10, want)
        assert got["exhausted_keys"] == 2 and got["live_keys"] == 3
        check_top(e, lid, T0 + 10, order, 2, ks=(1, 2, 3))
    # a deleted token bucket of key 0 (tag 0: written with the dead mark) is not live
    run_both(e, o, (np.array([0], np.uint64), np.array([1], np.int32), np.array([(T0 + 11) * NS], np.int64),
                    np.array([1], np.uint16), np.array([rl_amd.OP_RESET], np.uint8)))
    want, order = expected(o, 1, T0 + 11, lims)
    assert [x[1] for x in order] == [top, 9]
    check_census(e, 1, T0 + 11, want)
    check_top(e, 1, T0 + 11, order, 2, ks=(3,))
