"""rl_limiter_digest / rl_limiter_digest_device against the oracle's Redis keyspace, bit-exact.

The expected digests never come from the engine: they are rl_amd.digest_model over
PyOracle.keyspace(now) (the "rl:<key>:<W>" counters and "tb:<key>" hashes with their PEXPIRE
deadlines) and over the oracle's local-cache entries that reject at now, written as the engine's
cache word x = write time + ttl (sw_step_cache, rl_device.hpp). The traces are those of
test_gpu_usage.py with key hashes 0 and ~0 added; they end mid-window, so sliding-window keys
hold two live buckets.
"""
import ctypes

import numpy as np
import pytest

import rl_amd
from oracle.rl_oracle import PyOracle

pytestmark = pytest.mark.gpu

NS = 1_000_000
T0 = 1_700_000_000_000
TOP = (1 << 64) - 1
# (algo, max_permits, window_ms, refill_per_s, capacity, local_cache_ttl_ms)
LIMS = [(rl_amd.SW, 5, 1000, 0.0, 0, 0), (rl_amd.TB, 10, 1000, 5.0, 0, 0),
        (rl_amd.SW, 3, 500, 0.0, 0, 0), (rl_amd.TB, 4, 300, 20.0, 0, 0),
        (rl_amd.SW, 4, 2000, 0.0, 0, 400)]
N_KEYS = 300
SPANS = ((1, T0 + 350, T0 + 3350), (2, T0 + 3350, T0 + 6350))
END = T0 + 6350
LAGS = (0, 40, 250, 700, 2500)


def engine(capacity=1 << 12, **kw):
    e = rl_amd.Engine(max_batch=1 << 18, capacity=capacity, **kw)
    for l in LIMS:
        e.add_limiter(*l)
    return e


def trace(seed, t_lo, t_hi, n=25000):
    rng = np.random.default_rng(seed)
    lim = rng.integers(0, len(LIMS), n).astype(np.uint16)
    idx = rng.integers(0, N_KEYS, n)
    keys = idx.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + lim.astype(np.uint64)
    keys[idx == 0] = 0                                     # key hashes 0 and ~0 under every limiter
    keys[idx == 1] = TOP
    now = np.sort(rng.integers(t_lo * NS, t_hi * NS, n)).astype(np.int64)
    permits = rng.integers(1, 4, n).astype(np.int32)
    ops = np.zeros(n, np.uint8)
    ops[rng.random(n) < 0.01] = rl_amd.OP_RESET
    return keys, permits, now, lim, ops


def region_bits(e, lid):
    regions = e.limiter_slots(lid) // rl_amd.REGION_SLOTS
    assert regions >= 8 and regions & (regions - 1) == 0
    return regions.bit_length() - 1


def raw(d):
    return [(int(a), int(b), int(c)) for a, b, c in zip(d["entries"], d["sum"], d["xr"])]


def total_of(d):
    x = 0
    for v in d["xr"]:
        x ^= int(v)
    return int(d["entries"].sum()), int(d["sum"].astype(object).sum()) & TOP, x


class State:
    """One engine and one oracle after the same two traces; expected entries per (lag)."""

    def __init__(self):
        self.e, self.o = engine(), PyOracle()
        for l in LIMS:
            self.o.add_limiter(*l)
        self.traces = [trace(*s) for s in SPANS]
        for tr in self.traces:
            a, r, _, st = self.e.execute(*tr)
            wa, wr, _ = self.o.run(*tr)
            assert st == rl_amd.RL_OK
            np.testing.assert_array_equal(a, np.asarray(wa, np.uint8))
            np.testing.assert_array_equal(r, np.asarray(wr, np.int64))
        self._ent = {}

    def entries(self, lid, lag):
        """(keyspace entries, rejecting cache entries as (key_hash, x)) of limiter lid at END + lag."""
        if lag not in self._ent:
            now = END + lag
            ks = self.o.keyspace(now)
            per = {}
            for l in range(len(LIMS)):
                mx, ttl = LIMS[l][1], LIMS[l][5]
                cache = [(k, w + ttl) for (cl, k), (v, w) in self.o.cache.items()
                         if cl == l and v >= mx and now - w < ttl] if ttl else []
                per[l] = ([x for x in ks if x[0] == l], cache)
            self._ent[lag] = per
        return self._ent[lag][lid]

    def model(self, lid, lag, bits, cache, shards=1, shard=None):
        ent, ce = self.entries(lid, lag)
        if shard is not None:
            ent = [x for x in ent if int(rl_amd.owner_of(np.uint64(x[1]), shards)) == shard]
            ce = [x for x in ce if int(rl_amd.owner_of(np.uint64(x[0]), shards)) == shard]
        return rl_amd.digest_model(ent, ce if cache else [], shards, bits)


@pytest.fixture(scope="module")
def state():
    return State()


def device_digest(e, lid, now_ns, bits, cache):
    import torch
    out = torch.full((3 << bits,), 0x5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                              # (the fill runs on torch's stream)
    e.limiter_digest_device(lid, now_ns, bits, out, cache=cache)
    e.sync()
    return out.cpu().numpy().tobytes()


def check_all(e, state, lag, bit_sets=None, device=False):
    """Every limiter, bucket size and flag of engine e against the model at END + lag."""
    now_ns = (END + lag) * NS
    for lid in range(len(LIMS)):
        k = region_bits(e, lid)
        for bits in bit_sets or sorted({0, 1, 3, k}):
            for cache in (False, True):
                want = state.model(lid, lag, bits, cache)
                got, tot = e.limiter_digest(lid, now_ns, bits, cache=cache)
                assert raw(got) == raw(want), (lid, lag, bits, cache)
                assert tot == total_of(want), (lid, lag, bits, cache)
                if device:
                    assert device_digest(e, lid, now_ns, bits, cache) == got.tobytes(), (lid, lag, bits, cache)


@pytest.mark.parametrize("lag", LAGS)
def test_digests_match_the_model_over_the_oracle(state, lag):
    check_all(state.e, state, lag, device=True)
    n = {lid: len(state.entries(lid, lag)[0]) for lid in range(len(LIMS))}
    # the inputs keep the test from going hollow
    if lag == 0:
        keys0 = {x[1] for x in state.entries(0, 0)[0]}
        assert n[0] > len(keys0) > 200 and {0, TOP} <= keys0          # two live buckets per key
        assert all({0, TOP} <= {x[1] for x in state.entries(lid, 0)[0]} for lid in (1, 4))
        assert len(state.entries(4, 0)[1]) >= 10                      # rejecting cache entries
        with_c, without = (state.model(4, 0, 3, c) for c in (True, False))
        assert with_c.tobytes() != without.tobytes()
        assert min(state.model(0, 0, 3, False)["entries"]) > 0        # every bucket is populated
    if lag == 700:
        assert n[2] == 0 and n[3] == 0 and n[0] > 0 and not state.entries(4, lag)[1]
    if lag == 2500:
        assert not any(n.values())
        assert state.e.limiter_usage(0, (END + lag) * NS)["used_slots"] > 0   # tombstones


def test_bucket_bits_beyond_the_region_bits_and_other_bad_arguments(state):
    e, L = state.e, state.e._L
    bad = rl_amd.RL_E_INVALID_ARG
    k = region_bits(e, 0)
    out = np.zeros(2 << k, rl_amd.DIGEST_DTYPE)
    out.view(np.uint8)[:] = 0x5A
    before = out.tobytes()
    tot = rl_amd.BucketDigest(7, 7, 7)
    for lid, bits, flags in ((0, k + 1, 0), (0, k + 1, 1), (0, 64, 0), (len(LIMS), 0, 0), (0, 0, 2), (0, 3, 0x80000001)):
        assert L.rl_limiter_digest(e._h, lid, END * NS, bits, flags, rl_amd._p(out), ctypes.byref(tot)) == bad
    assert L.rl_limiter_digest(e._h, 0, END * NS, 0, 0, None, ctypes.byref(tot)) == bad
    assert out.tobytes() == before and (tot.entries, tot.sum, tot.xr) == (7, 7, 7)
    import torch
    dev = torch.full((3 << (k + 1),), 0x5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L.rl_limiter_digest_device(e._h, 0, END * NS, k + 1, 0, rl_amd._p(dev), None) == bad
    assert L.rl_limiter_digest_device(e._h, len(LIMS), END * NS, 0, 0, rl_amd._p(dev), None) == bad
    assert L.rl_limiter_digest_device(e._h, 0, END * NS, 0, 4, rl_amd._p(dev), None) == bad
    assert L.rl_limiter_digest_device(e._h, 0, END * NS, 0, 0, None, None) == bad
    assert L.rl_limiter_digest_device(e._h, 0, END * NS, 0, 0, ctypes.c_void_p(dev.data_ptr() + 4), None) == bad
    e.sync()
    assert bool((dev == 0x5A5A).all())
    with pytest.raises(rl_amd.RlError) as x:
        e.limiter_digest(0, END * NS, k + 1)
    assert x.value.status == bad
    assert e.limiter_digest(0, END * NS, k)[0].shape == (1 << k,)     # the largest allowed


def replay(e, state):
    for tr in state.traces:
        assert e.execute(*tr)[3] == rl_amd.RL_OK


def test_the_result_does_not_depend_on_the_grid(state):
    e = engine()
    replay(e, state)
    now_ns = (END + 40) * NS

    def sweep_grids(lid, bit_set, grids):
        for bits in bit_set:
            for cache in (False, True):
                want = state.model(lid, 40, bits, cache)
                for per_cu in grids:
                    e.tune("digest_per_cu", per_cu)
                    assert raw(e.limiter_digest(lid, now_ns, bits, cache=cache)[0]) == raw(want), \
                        (lid, bits, cache, per_cu)
                    assert device_digest(e, lid, now_ns, bits, cache) == want.tobytes()
        e.tune("digest_per_cu", 0)

    for lid in range(len(LIMS)):
        sweep_grids(lid, (0, 3, region_bits(e, lid)), (1, 0))
    # 2^16 slots = 256 regions
    for lid in (0, 4):
        e.grow_limiter(lid, 1 << 15)
        assert e.limiter_slots(lid) >= 1 << 16
        k = region_bits(e, lid)
        sweep_grids(lid, (0, 3, k - 1, k), (1, 0))
    # 2^22 slots = 16384 regions: more regions than waves at one workgroup per CU, so a wave's
    # span holds several regions and crosses bucket boundaries; at 3 or 5 per CU the spans are
    # no power of two, so they start and end inside buckets (atomics and plain stores mix)
    e.grow_limiter(4, 1 << 21)
    assert e.limiter_slots(4) >= 1 << 22
    k = region_bits(e, 4)
    sweep_grids(4, (0, 3, 9, k - 3, k - 1, k), (1, 3, 5, 0))
    with pytest.raises(rl_amd.RlError):
        e.tune("digest_per_cu", -1)


def test_grow_sweep_shrink_and_restore_leave_the_digests_alone(state):
    lag = 250                                             # limiters 2 and 3 are partly dead by now
    now_ns = (END + lag) * NS
    assert 0 < len(state.entries(3, lag)[0]) < len(state.entries(3, 0)[0])
    a = engine()
    replay(a, state)
    check_all(a, state, lag, bit_sets=(0, 3))
    for lid in range(len(LIMS)):
        for _ in range(4):
            a.grow_limiter(lid, a.limiter_slots(lid))
        assert a.limiter_slots(lid) >= 16 * state.e.limiter_slots(lid)
    check_all(a, state, lag)
    assert a.sweep_expired(now_ns) > 0
    check_all(a, state, lag)
    for lid in range(len(LIMS)):
        assert a.shrink_limiter(lid, now_ns)["halvings"] > 0
    check_all(a, state, lag)
    # engine B: tables of another region count, filled from A's snapshot
    b = engine(capacity=1 << 14)
    for lid in range(len(LIMS)):
        assert b.limiter_slots(lid) != a.limiter_slots(lid)
        for chunk in a.snapshot(lid):
            st, n = b.restore_keys(chunk)
            assert st == rl_amd.RL_OK and n == chunk.shape[0]
    check_all(b, state, lag)
    for lid in range(len(LIMS)):
        for cache in (False, True):
            da, ta = a.limiter_digest(lid, now_ns, 3, cache=cache)
            db, tb = b.limiter_digest(lid, now_ns, 3, cache=cache)
            assert da.tobytes() == db.tobytes() and ta == tb


def test_a_change_shows_in_exactly_the_keys_bucket(state):
    e = engine()
    replay(e, state)
    now = END + 10
    bits = 3

    def digests():
        return {(lid, c): e.limiter_digest(lid, now * NS, bits, cache=c)[0]
                for lid in range(len(LIMS)) for c in (False, True)}

    def bucket_of(key):
        d = rl_amd.digest_model([(0, key, 0, 0, 1, 0.0, 0, 1)], [], 1, bits)
        (b,) = np.nonzero(d["entries"])[0]
        return int(b)

    def changed(before, after):
        return {(lid, c, b) for (lid, c) in before for b in range(1 << bits)
                if before[lid, c][b].tobytes() != after[lid, c][b].tobytes()}

    def run(key, lid, op=rl_amd.OP_ACQUIRE, permits=1):
        a, r, _, st = e.execute(np.array([key], np.uint64), np.array([permits], np.int32),
                                np.array([now * NS], np.int64), np.array([lid], np.uint16),
                                np.array([op], np.uint8))
        assert st == rl_amd.RL_OK
        return int(a[0])

    d0 = digests()
    fresh = 0xDEADBEEFCAFEF00D
    for lid in (0, 1):                                    # one more acquire: SW and TB
        assert run(fresh, lid) == 1
        d1 = digests()
        assert changed(d0, d1) == {(lid, False, bucket_of(fresh)), (lid, True, bucket_of(fresh))}
        assert d1[lid, False]["entries"][bucket_of(fresh)] == d0[lid, False]["entries"][bucket_of(fresh)] + 1
        d0 = d1
    assert run(fresh, 0) == 1                             # the same key again: the count changes
    d1 = digests()
    assert changed(d0, d1) == {(0, c, bucket_of(fresh)) for c in (False, True)}
    assert d1[0, False]["entries"].tolist() == d0[0, False]["entries"].tolist()
    d0 = d1
    # a denied acquire changes nothing: sliding window at its limit, token bucket drained
    for _ in range(3):
        assert run(fresh, 0) == 1
    d0 = digests()
    assert run(fresh, 0) == 0
    assert run(fresh, 1, permits=10) == 0                 # 9 tokens left of 10
    assert changed(d0, digests()) == set()
    # a peek changes nothing
    for lid in range(len(LIMS)):
        e.available(lid, np.array([fresh, 0, TOP], np.uint64), now * NS)
    assert changed(d0, digests()) == set()
    # a reset of a live key changes exactly its bucket
    live = state.entries(0, 10)[0][len(state.entries(0, 10)[0]) // 2][1]
    run(live, 0, op=rl_amd.OP_RESET)
    d1 = digests()
    assert changed(d0, d1) == {(0, c, bucket_of(live)) for c in (False, True)}
    assert d1[0, False]["entries"][bucket_of(live)] < d0[0, False]["entries"][bucket_of(live)]


def test_each_shard_digests_its_own_keys(state):
    tot = 0
    for s in (0, 1):
        e = engine(shard_index=s, shard_count=2)
        for tr in state.traces:
            m = rl_amd.owner_of(tr[0], 2) == s
            assert 0 < m.sum() < m.shape[0]
            assert e.execute(*(x[m] for x in tr))[3] == rl_amd.RL_OK
        for lid in range(len(LIMS)):
            for bits in (0, 3, region_bits(e, lid)):
                for cache in (False, True):
                    want = state.model(lid, 40, bits, cache, shards=2, shard=s)
                    got, _ = e.limiter_digest(lid, (END + 40) * NS, bits, cache=cache)
                    assert raw(got) == raw(want), (s, lid, bits, cache)
        tot += e.limiter_digest(0, (END + 40) * NS, 0)[1][0]
    assert tot == state.e.limiter_digest(0, (END + 40) * NS, 0)[1][0] > 0
    # the restriction is not hollow: both shards hold entries, in other buckets than unsharded
    halves = [state.model(0, 40, 3, True, shards=2, shard=s) for s in (0, 1)]
    assert all(h["entries"].sum() > 50 for h in halves)
    assert raw(halves[0]) != raw(state.model(0, 40, 3, True))


@pytest.mark.parametrize("pipeline", [False, True])
def test_the_calls_only_read_and_run_behind_the_batches(state, pipeline):
    import torch
    e = engine(pipeline=pipeline)
    assert e.execute(*state.traces[0])[3] == rl_amd.RL_OK
    now_ns = SPANS[0][2] * NS
    before = (e.stats(), e.last_status(), e.export_state(now_ns).tobytes())
    for lid in range(len(LIMS)):
        for bits in (0, 3):
            got, _ = e.limiter_digest(lid, now_ns, bits)
            assert device_digest(e, lid, now_ns, bits, True) == got.tobytes()
    assert (e.stats(), e.last_status(), e.export_state(now_ns).tobytes()) == before
    # the next segment as a device batch with one invalid request, not waited for and its
    # status not collected: the digests run behind it and leave the status pending
    tr = [np.concatenate([x, x[-1:]]) for x in state.traces[1]]
    tr[1][-1] = 0                                         # permits 0: RL_E_INVALID_REQUEST
    n = tr[0].shape[0]
    dev = [torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else
                            x.view(np.int16) if x.dtype == np.uint16 else x).cuda() for x in tr]
    allowed = torch.zeros(n, dtype=torch.uint8, device="cuda")
    remaining = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.execute_device(n, *dev, allowed, remaining)
    got = {(lid, c): e.limiter_digest(lid, END * NS, 3, cache=c)[0] for lid in range(len(LIMS))
           for c in (False, True)}
    dgot = {lid: device_digest(e, lid, END * NS, 3, True) for lid in range(len(LIMS))}
    assert e.last_status() == rl_amd.RL_E_INVALID_REQUEST
    for (lid, c), d in got.items():
        assert raw(d) == raw(state.model(lid, 0, 3, c)), (lid, c)
    for lid, d in dgot.items():
        assert d == got[lid, True].tobytes()
