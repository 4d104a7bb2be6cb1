"""rl_quota on the GPU: exact equality, on every query, with the definition evaluated on the
oracle (tests/quota_cases.py: remaining = the oracle's peek at now, reset = the first t of a FULL
scan of now .. now + 2w + 2 at which the peek reads maxPermits, retry = the first t at which one
acquire on a copy of the key's state is allowed; the scans rely on no monotonicity and assert it).
The layout is that of tests/test_gpu_retry_after.py: seven limiters (its five and two sparse sliding
windows), 12 keys plus one untouched key each, query times at the trace end + {0, 1, 37, w}. The
larger growth / tombstone case uses the bracket on the C oracle instead: RL_OP_PEEK at
now + r - 1 reads < max and at now + r reads max.

The identity case needs a state in which reset and retry-after of maxPermits differ, that is a
rejecting cache entry that outlives the key's counters. The seven traces leave rejecting entries at
the query times but none that does (a key over its limit keeps its counters for longer than the
50 ms an entry lives), so that case adds one short burst on a fresh key per cache-on limiter,
built so that the entry is written late in the counters' life; it is asserted on the oracle first."""
import copy

import numpy as np
import pytest

import quota_cases as qc
import rl_amd
from oracle.coracle import COracle

NS, T0 = qc.NS, qc.T0
CASES = qc.CASES
NEVER, INVALID = rl_amd.RETRY_NEVER, rl_amd.QUOTA_INVALID
CACHE_OFF = [lid for lid, c in enumerate(CASES) if c[0][4] == 0]
CACHE_ON = [lid for lid, c in enumerate(CASES) if c[0][4] != 0]


def new_engine(**kw):
    e = rl_amd.Engine(max_batch=1 << 16, capacity=1 << 10, **kw)
    for (algo, mx, w, rate, ttl), *_ in CASES:
        e.add_limiter(algo, mx, w, rate, local_cache_ttl_ms=ttl)
    return e


def feed(e):
    for lid in range(len(CASES)):
        a, r, _, st = e.execute(*qc.lim_trace(lid), want_tokens=False)
        assert st == rl_amd.RL_OK
    return e


@pytest.fixture(scope="module")
def oracle():
    return qc.new_oracle()


@pytest.fixture(scope="module")
def reference(oracle):
    """Per limiter: its query set and the expected answers (computed once, never changed)."""
    ref = qc.build_reference(oracle)
    qc.check_not_vacuous(ref)          # the set must not pass vacuously (the oracle's answers alone)
    return ref


@pytest.fixture(scope="module")
def fed_engine():
    """An engine after the seven traces, for the tests that only query it."""
    e = feed(new_engine())
    yield e
    e.close()


def _all(reference):
    cat = lambda f: np.concatenate([d[f] for d in reference])  # noqa: E731
    return tuple(cat(f) for f in ("keys", "permits", "now_ns", "limiter", "remaining", "reset", "retry"))


def _mismatch(name, got, want, k, t):
    bad = np.nonzero(got != want)[0]
    return f"{name}: {bad.size} of {len(want)} differ, first: " + ", ".join(
        f"[{i}] key {int(k[i]):#x} now {t[i] // NS}: got {got[i]} want {want[i]}" for i in bad[:5])


def _same(got, want, k, t):
    for name, g, w in zip(("remaining", "reset_ms", "retry_ms"), got, want):
        assert np.array_equal(g, w), _mismatch(name, g, w, k, t)


pytestmark = pytest.mark.gpu


# ---- 1. seven small limiters
@pytest.mark.parametrize("lid", range(len(CASES)))
def test_each_limiter_equals_the_scan(fed_engine, reference, lid):
    d = reference[lid]
    k, p, t, l = d["keys"], d["permits"], d["now_ns"], d["limiter"]
    rem, rst, rty, st = fed_engine.quota(l, k, t, p)
    assert st == rl_amd.RL_OK
    _same((rem, rst, rty), (d["remaining"], d["reset"], d["retry"]), k, t)
    wait, st = fed_engine.retry_after(l, k, p, t)
    assert st == rl_amd.RL_OK and np.array_equal(rty, wait)
    w = CASES[lid][0][2]
    assert rst.min() >= 0 and rst.max() <= 2 * w + 1
    # a scalar limiter id and NULL limiter / permits / skip take the same path as the arrays
    if lid == 0:
        r1, r2 = np.zeros(len(k), np.int64), np.zeros(len(k), np.int64)
        st = fed_engine._L.rl_quota(fed_engine.handle, len(k), rl_amd._p(k), rl_amd._p(t), None, None, None,
                                    rl_amd._p(r1), rl_amd._p(r2), None)
        assert st == rl_amd.RL_OK and np.array_equal(r1, d["remaining"]) and np.array_equal(r2, d["reset"])


# ---- 2. the identity: reset is retry-after of maxPermits with the local cache ignored
def _late_entry_burst(lid):
    """A fresh key of cache-on limiter lid: max acquires early in a window W, one more (denied,
    so it writes a rejecting entry) 30 ms before the window ends. The counters lapse at
    W + 5 + w + 1, the entry 14 ms later. Returns the burst and queries around the lapse."""
    (_, mx, w, _, ttl), *_ = CASES[lid]
    key = qc.mix64(np.array([qc.N_KEYS + 7], np.uint64) + np.uint64((lid + 1) << 32))[0]
    W = ((qc.trace_end(lid) + 2 * w) // w + 1) * w
    at = [W + 5] * mx + [W + w - 30]
    n = len(at)
    burst = (np.full(n, key, np.uint64), np.ones(n, np.int32), np.array(at, np.int64) * NS,
             np.full(n, lid, np.uint16))
    times = [W + w - 10, W + w + 3, W + w + 5, W + w + 6, W + w + 19, W + w + 20]
    assert times[0] < W + w - 30 + ttl and times[-1] == W + w - 30 + ttl
    return key, burst, times


def test_reset_is_retry_after_of_max_without_the_cache(oracle, reference):
    e = feed(new_engine())
    for lid in CACHE_OFF:
        d = reference[lid]
        mx = CASES[lid][0][1]
        assert np.array_equal(d["pair_reset"], d["pair_retry_max"]), lid          # on the oracle
        _, rst, _, st = e.quota(lid, d["pair_keys"], d["pair_now_ns"])
        wait, st2 = e.retry_after(lid, d["pair_keys"], mx, d["pair_now_ns"])
        assert st == rl_amd.RL_OK and st2 == rl_amd.RL_OK
        assert np.array_equal(rst, d["pair_reset"]) and np.array_equal(rst, wait), lid
    o = copy.deepcopy(oracle)
    for lid in CACHE_ON:
        mx = CASES[lid][0][1]
        key, burst, times = _late_entry_burst(lid)
        wa, _, _ = o.run(*burst)
        assert list(wa) == [1] * mx + [0]
        want = [qc.scan_quota(o, lid, int(key), (mx,), now) for now in times]
        w_rem = np.array([x[0] for x in want], np.int64)
        w_rst = np.array([x[1] for x in want], np.int64)
        w_max = np.array([x[2][0] for x in want], np.int64)
        # on the oracle first: the entry delays the acquire, not the quota
        assert (w_rst != w_max).sum() >= 3 and (w_rst < w_max).sum() == (w_rst != w_max).sum(), (lid, w_rst, w_max)
        assert (w_rst > 0).sum() >= 2 and (w_rst == 0).sum() >= 2
        a, _, _, st = e.execute(*burst, want_tokens=False)
        assert st == rl_amd.RL_OK and list(a) == list(wa)
        k = np.full(len(times), key, np.uint64)
        t = np.array(times, np.int64) * NS
        rem, rst, rty, st = e.quota(lid, k, t, mx)
        wait, st2 = e.retry_after(lid, k, mx, t)
        assert st == rl_amd.RL_OK and st2 == rl_amd.RL_OK
        _same((rem, rst, rty), (w_rem, w_rst, w_max), k, t)
        assert np.array_equal(wait, w_max) and (rst != wait).sum() >= 3
    e.close()


# ---- 3. one call mixing all seven limiters, with invalid entries; the argument rules
def test_mixed_call_with_invalid_entries(fed_engine, reference):
    k, p, t, l, w_rem, w_rst, w_rty = _all(reference)
    perm = np.random.default_rng(5).permutation(len(k))
    k, p, t, l, w_rem, w_rst, w_rty = (x[perm] for x in (k, p, t, l, w_rem, w_rst, w_rty))
    rem, rst, rty, st = fed_engine.quota(l, k, t, p)
    assert st == rl_amd.RL_OK
    _same((rem, rst, rty), (w_rem, w_rst, w_rty), k, t)
    # without permits: remaining and reset only
    rem, rst, rty, st = fed_engine.quota(l, k, t)
    assert st == rl_amd.RL_OK and rty is None
    _same((rem, rst), (w_rem, w_rst), k, t)
    # permits 0, permits -3, limiter 99: -2 in all three outputs, RL_E_INVALID_REQUEST, the rest unchanged
    at = [3, len(k) // 2, len(k) - 1]
    k2 = np.insert(k, at, k[at])
    t2 = np.insert(t, at, t[at])
    p2 = np.insert(p, at, [0, -3, 1])
    l2 = np.insert(l, at, [l[at[0]], l[at[1]], 99])
    bad = np.zeros(len(k2), bool)
    bad[[at[0], at[1] + 1, at[2] + 2]] = True
    assert list(p2[bad]) == [0, -3, 1] and l2[bad][2] == 99
    rem, rst, rty, st = fed_engine.quota(l2, k2, t2, p2)
    assert st == rl_amd.RL_E_INVALID_REQUEST
    for out in (rem, rst, rty):
        assert np.all(out[bad] == INVALID)
    _same((rem[~bad], rst[~bad], rty[~bad]), (w_rem, w_rst, w_rty), k, t)
    # without permits only the unknown limiter is invalid
    rem, rst, _, st = fed_engine.quota(l2, k2, t2)
    assert st == rl_amd.RL_E_INVALID_REQUEST
    only = np.zeros(len(k2), bool)
    only[at[2] + 2] = True
    assert np.all(rem[only] == INVALID) and np.all(rst[only] == INVALID)
    assert np.all(rst[~only] >= 0) and np.array_equal(rst[~bad], w_rst)
    # argument errors of the host entry: outputs untouched
    L, h, P = fed_engine._L, fed_engine.handle, rl_amd._p
    o1, o2, o3 = (np.full(4, 77, np.int64) for _ in range(3))
    sk = np.zeros(4, np.uint8)
    bad_arg = rl_amd.RL_E_INVALID_ARG
    assert L.rl_quota(h, 4, None, P(t), None, None, None, P(o1), P(o2), None) == bad_arg
    assert L.rl_quota(h, 4, P(k), None, None, None, None, P(o1), P(o2), None) == bad_arg
    assert L.rl_quota(h, 4, P(k), P(t), None, None, None, None, P(o2), None) == bad_arg
    assert L.rl_quota(h, 4, P(k), P(t), None, None, None, P(o1), None, None) == bad_arg
    assert L.rl_quota(h, 4, P(k), P(t), None, P(p), None, P(o1), P(o2), None) == bad_arg      # permits, no retry_ms
    assert L.rl_quota(h, 4, P(k), P(t), None, None, None, P(o1), P(o2), P(o3)) == bad_arg     # retry_ms, no permits
    assert L.rl_quota(h, 4, P(k), P(t), None, None, P(sk), P(o1), P(o2), None) == bad_arg     # skip, no permits
    assert L.rl_quota_device(h, 4, P(k), P(t), None, P(p), None, P(o1), P(o2), None, None) == bad_arg
    assert L.rl_quota_device(h, 4, P(k), P(t), None, None, P(sk), P(o1), P(o2), None, None) == bad_arg
    assert L.rl_quota(h, (1 << 16) + 1, P(k), P(t), None, None, None, P(o1), P(o2), None) == rl_amd.RL_E_TOO_LARGE
    assert L.rl_quota_device(h, (1 << 16) + 1, P(k), P(t), None, None, None, P(o1), P(o2), None,
                             None) == rl_amd.RL_E_TOO_LARGE
    assert L.rl_quota(h, 0, None, None, None, None, None, None, None, None) == rl_amd.RL_OK
    assert L.rl_quota_device(h, 0, None, None, None, None, None, None, None, None, None) == rl_amd.RL_OK
    assert all(np.all(o == 77) for o in (o1, o2, o3))


def _end_batch(dt=0):
    """One acquire per (limiter, key, query permits) at the limiter's trace end + dt."""
    k, p, t, l = [], [], [], []
    for lid in range(len(CASES)):
        for key in qc.lim_keys(lid):
            for pp in CASES[lid][4][:3]:
                k.append(key); p.append(pp); t.append((qc.trace_end(lid) + dt) * NS); l.append(lid)
    o = np.argsort(np.array(t), kind="stable")
    return (np.array(k, np.uint64)[o], np.array(p, np.int32)[o], np.array(t, np.int64)[o],
            np.array(l, np.uint16)[o])


# ---- 4. skip
def test_skip_takes_a_batchs_allowed():
    e = feed(new_engine())
    k, p, t, l = _end_batch()
    a, r, _, st = e.execute(k, p, t, l, want_tokens=False)
    assert st == rl_amd.RL_OK
    assert 0.1 * len(a) < a.sum() < 0.9 * len(a)
    rem, rst, plain, st1 = e.quota(l, k, t, p)
    rem2, rst2, skipped, st2 = e.quota(l, k, t, p, skip=a)
    assert st1 == rl_amd.RL_OK and st2 == rl_amd.RL_OK
    assert np.all(skipped[a != 0] == 0)
    assert np.array_equal(skipped[a == 0], plain[a == 0])
    assert (plain[a != 0] > 0).sum() > 0          # the skip did skip: those are not 0 by themselves
    assert (plain[a == 0] > 0).sum() > 0
    # remaining and reset are answered for skipped queries too
    assert np.array_equal(rem2, rem) and np.array_equal(rst2, rst)
    assert (rst[a != 0] > 0).sum() > 0 and (rem[a != 0] > 0).sum() > 0
    # a skipped entry's permits is not looked at, invalid or not
    p2 = p.copy()
    p2[a != 0] = 0
    rem3, rst3, again, st3 = e.quota(l, k, t, p2, skip=a)
    assert st3 == rl_amd.RL_OK and np.array_equal(again, skipped)
    assert np.array_equal(rem3, rem) and np.array_equal(rst3, rst)
    e.close()


# ---- 5. read-only
def test_queries_change_nothing(oracle, reference):
    e = feed(new_engine())
    at = max(qc.trace_end(lid) for lid in range(len(CASES))) * NS
    order = ["limiter", "key_hash", "kind", "window_start_ms"]
    before = np.sort(e.export_state(at), order=order)
    stats0, status0 = e.stats(), e.last_status()
    for d in reference:
        rem, rst, rty, _ = e.quota(d["limiter"], d["keys"], d["now_ns"], d["permits"])
        _same((rem, rst, rty), (d["remaining"], d["reset"], d["retry"]), d["keys"], d["now_ns"])
        rem, rst, _, _ = e.quota(d["limiter"], d["keys"], d["now_ns"])
        assert np.array_equal(rst, d["reset"])
    assert e.stats() == stats0 and e.last_status() == status0
    after = np.sort(e.export_state(at), order=order)
    assert before.size > 0 and np.array_equal(before, after)
    # remaining is what rl_available reads (a peek batch: in time order per limiter)
    for lid, d in enumerate(reference):
        od = np.argsort(d["pair_now_ns"], kind="stable")
        avail, st = e.available(lid, d["pair_keys"][od], d["pair_now_ns"][od])
        rem, _, _, st2 = e.quota(lid, d["pair_keys"][od], d["pair_now_ns"][od])
        assert st == rl_amd.RL_OK and st2 == rl_amd.RL_OK and np.array_equal(rem, avail), lid
    # the next batch still matches the oracle, the cache-on limiters' cache hits included
    o = copy.deepcopy(oracle)
    k, p, t, l = _end_batch(dt=2)
    k, p, t, l = np.repeat(k, 2), np.repeat(p, 2), np.repeat(t, 2), np.repeat(l, 2)
    hits0 = o.cache_hits
    wa, wr, _ = o.run(k, p, t, l)
    a, r, _, st = e.execute(k, p, t, l, want_tokens=False)
    assert st == rl_amd.RL_OK
    assert np.array_equal(a, np.array(wa, np.uint8)) and np.array_equal(r, np.array(wr, np.int64))
    assert o.cache_hits - hits0 > 0
    assert e.stats()["cache_hits"] == o.cache_hits - hits0
    e.close()


# ---- 6. probing, tombstones, growth
def test_growth_and_dead_slots_bracket():
    lim = [rl_amd.TB, 5, 1000, 10.0]
    e = rl_amd.Engine(max_batch=1 << 18, capacity=1)
    e.add_limiter(*lim, capacity=1)
    o = COracle([lim])
    rng = np.random.default_rng(21)
    n_first, n_req = 20_000, 100_000
    first = rl_amd.mix64(np.arange(n_first, dtype=np.uint64) + np.uint64(9 << 40))
    # new keys come in as fast as the table may grow (about 1/8 of it per batch); every batch
    # also revisits the keys seen so far, until all 20k keys are in and 100k requests made
    known, done, t = 0, 0, T0
    while known < n_first or done < n_req:
        fresh = min(e.limiter_slots(0) // 8, n_first - known)
        ranks = np.concatenate([np.arange(known, known + fresh),
                                rng.integers(0, known + fresh, 3000 if known else 0)])
        ranks = ranks[rng.permutation(len(ranks))]
        known += fresh
        k = first[ranks]
        p = rng.integers(1, 4, len(k)).astype(np.int32)
        now = (t * NS + np.sort(rng.integers(0, 20 * NS, len(k)))).astype(np.int64)
        t += 20
        a, r, _, st = e.execute(k, p, now, want_tokens=False)
        assert st == rl_amd.RL_OK
        wa, wr, _, _ = o.run(k, p, now, want_tokens=False)
        assert np.array_equal(a, wa) and np.array_equal(r, wr)
        done += len(k)
    assert known == n_first and e.stats()["table_grows"] >= 1
    # 3 w later, other keys: the regions this batch loads drop the first keys' dead slots,
    # the ones it probes bucket by bucket keep them as tombstones
    other = rl_amd.mix64(np.arange(6000, dtype=np.uint64) + np.uint64(10 << 40))
    t2 = t + 3000
    k = other[rng.integers(0, len(other), 24_000)]
    p = rng.integers(1, 4, len(k)).astype(np.int32)
    now = (t2 * NS + np.sort(rng.integers(0, 300 * NS, len(k)))).astype(np.int64)
    a, r, _, st = e.execute(k, p, now, want_tokens=False)
    wa, wr, _, _ = o.run(k, p, now, want_tokens=False)
    assert st == rl_amd.RL_OK and np.array_equal(a, wa) and np.array_equal(r, wr)
    # 4096 queries over both sets, shortly after
    qk = np.concatenate([first[rng.integers(0, n_first, 2048)], other[rng.integers(0, len(other), 2048)]])
    qp = rng.integers(1, 7, len(qk)).astype(np.int32)             # 6 > max: never
    qt = ((t2 + 300) * NS + rng.integers(0, 50 * NS, len(qk))).astype(np.int64)
    rem, got, rty, st = e.quota(0, qk, qt, qp)
    assert st == rl_amd.RL_OK
    wait, st = e.retry_after(0, qk, qp, qt)
    assert st == rl_amd.RL_OK and np.array_equal(rty, wait)
    assert (got > 0).sum() > 400 and (got == 0).sum() > 400
    assert got.min() >= 0 and got.max() <= 2 * 1000 + 1
    # the bracket: peeks (remaining = (long) balance) at now, now + r - 1 and now + r, in time order
    now_ms = qt // NS
    pk = np.concatenate([qk, qk, qk])
    pt = np.concatenate([now_ms, now_ms + got - 1, now_ms + got]) * NS
    side = np.repeat(np.array([0, 1, 2]), len(qk))
    first_ms = np.tile(got == 0, 3)                               # r = 0: no t - 1 to refute
    want_now = np.tile(rem, 3)
    od = np.argsort(pt, kind="stable")
    _, peek, _, _ = o.run(pk[od], np.ones(len(od), np.int32), pt[od].astype(np.int64),
                          ops=np.full(len(od), rl_amd.OP_PEEK, np.uint8), want_tokens=False)
    ok = np.select([side[od] == 0, side[od] == 1], [peek == want_now[od], (peek < 5) | first_ms[od]], peek == 5)
    assert ok.all(), f"{(~ok).sum()} bracket failures"
    e.close()
    o.close()


# ---- 7. device entry
def _dev(*arrays):
    import torch
    out = []
    for x in arrays:
        x = np.array(x)                               # (a writable copy: the reference is read-only)
        x = x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int16) if x.dtype == np.uint16 else x
        out.append(torch.from_numpy(x).cuda())
    return out


def test_device_entry_equals_host_entry(fed_engine, reference):
    import torch
    k, p, t, l, w_rem, w_rst, w_rty = _all(reference)
    skip = (np.arange(len(k)) % 3 == 0).astype(np.uint8)
    h_rem, h_rst, h_rty, _ = fed_engine.quota(l, k, t, p, skip=skip)
    assert np.array_equal(h_rem, w_rem) and np.array_equal(h_rst, w_rst)
    assert np.array_equal(h_rty[skip == 0], w_rty[skip == 0]) and np.all(h_rty[skip != 0] == 0)
    dk, dt, dl, dp, ds = _dev(k, t, l, p, skip)
    n = len(k)
    out = [torch.full((n,), 77, dtype=torch.int64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    fed_engine.quota_device(n, dk, dt, dl, dp, ds, *out)
    fed_engine.sync()
    for got, want in zip(out, (h_rem, h_rst, h_rty)):
        assert np.array_equal(got.cpu().numpy(), want)
    # on a caller's stream: ordered behind its work, and its later work behind the query; once
    # with permits and no skip, once without permits
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        o1 = [torch.full((n,), 77, dtype=torch.int64, device="cuda") for _ in range(3)]
        fed_engine.quota_device(n, dk, dt, dl, dp, None, *o1, stream=s.cuda_stream)
        c1 = [x.clone() for x in o1]
        o2 = [torch.full((n,), 77, dtype=torch.int64, device="cuda") for _ in range(2)]
        fed_engine.quota_device(n, dk, dt, dl, None, None, o2[0], o2[1], None, stream=s.cuda_stream)
        c2 = [x.clone() for x in o2]
    s.synchronize()
    for got, want in zip(c1, (w_rem, w_rst, w_rty)):
        assert np.array_equal(got.cpu().numpy(), want)
    for got, want in zip(c2, (w_rem, w_rst)):
        assert np.array_equal(got.cpu().numpy(), want)
    assert fed_engine.last_status() == rl_amd.RL_OK


def test_device_query_is_ordered_behind_a_pipelined_batch(reference):
    """RL_OPT_PIPELINE: a query enqueued right after a device batch sees that batch."""
    import torch
    e = new_engine(pipeline=True)
    for lid in range(len(CASES)):
        k, p, t, l = qc.lim_trace(lid)
        dev = _dev(k, p, t, l)
        a = torch.empty(len(k), dtype=torch.uint8, device="cuda")
        r = torch.empty(len(k), dtype=torch.int64, device="cuda")
        d = reference[lid]
        qk, qt, ql, qp = _dev(d["keys"], d["now_ns"], d["limiter"], d["permits"])
        out = [torch.empty(len(d["keys"]), dtype=torch.int64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        e.execute_device(len(k), *dev, None, a, r)
        e.quota_device(len(d["keys"]), qk, qt, ql, qp, None, *out)
        assert e.last_status() == rl_amd.RL_OK
        for got, f in zip(out, ("remaining", "reset", "retry")):
            assert np.array_equal(got.cpu().numpy(), d[f]), (lid, f)
    e.close()


# ---- 8. end to end
def test_max_permits_are_denied_one_ms_before_and_allowed_at_the_reset(oracle, reference):
    picks, seen = [], set()
    for lid, d in enumerate(reference):
        mx = CASES[lid][0][1]
        for i in np.nonzero(d["pair_reset"] > 0)[0]:
            key = int(d["pair_keys"][i])
            if (lid, key) in seen:
                continue
            # on the oracle: denied at now + reset - 1, then allowed at now + reset (with the local
            # cache a denial may itself set a rejecting entry, and a live entry rejects whatever
            # the counters say; such a pair is not a test of the quota)
            o = copy.deepcopy(oracle)
            at = int(d["pair_now_ns"][i]) // NS + int(d["pair_reset"][i])
            wa, _, _ = o.run([key] * 2, [mx] * 2, [(at - 1) * NS, at * NS], [lid] * 2)
            if list(wa) == [0, 1]:
                seen.add((lid, key))
                picks.append((key, mx, at, lid))
    assert len(picks) >= 32, len(picks)
    k = np.repeat(np.array([x[0] for x in picks], np.uint64), 2)
    p = np.repeat(np.array([x[1] for x in picks], np.int32), 2)
    l = np.repeat(np.array([x[3] for x in picks], np.uint16), 2)
    t = np.array([[(x[2] - 1) * NS, x[2] * NS] for x in picks], np.int64).ravel()
    od = np.argsort(t, kind="stable")
    e = feed(new_engine())
    a, _, _, st = e.execute(k[od], p[od], t[od], l[od], want_tokens=False)
    assert st == rl_amd.RL_OK
    back = np.empty_like(a)
    back[od] = a
    assert np.array_equal(back, np.tile(np.array([0, 1], np.uint8), len(picks)))
    e.close()
