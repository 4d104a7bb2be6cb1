"""rl_retry_after on the GPU: exact equality, on every query, with the definition evaluated on
the oracle. For a query (limiter, key, permits, now) the expected wait is the first t in a FULL
scan of now .. now + 2w + ttl + 2 at which one acquire on a copy of the oracle's state is
allowed (oracle.rl_oracle.PyOracle; the scan relies on no monotonicity and asserts that no
denial follows the first allow). The larger growth / tombstone case uses the bracket on the C
oracle instead: RL_OP_PEEK at now + r - 1 reads < p and at now + r reads >= p."""
import copy

import numpy as np
import pytest

import rl_amd
from oracle.coracle import COracle
from oracle.rl_oracle import PyOracle

NS = 1_000_000
T0 = 1_700_000_000_000
NEVER, INVALID = rl_amd.RETRY_NEVER, rl_amd.RETRY_INVALID

# (algo, max, window ms, refill/s, cache ttl ms), requests, span ms, trace permits hi, query permits
CASES = [
    ((rl_amd.TB, 5, 1000, 10.0, 0), 1500, 2000, 3, (1, 3, 5, 6)),
    ((rl_amd.TB, 5, 300, 0.5, 0), 600, 1000, 3, (1, 3, 5, 6)),      # expiry before refill
    ((rl_amd.TB, 7, 1000, 3.3, 0), 1500, 2000, 3, (1, 2, 7, 8)),
    ((rl_amd.SW, 10, 200, 0.0, 0), 1500, 500, 2, (1, 4, 10, 11)),
    ((rl_amd.SW, 10, 200, 0.0, 50), 1500, 500, 2, (1, 4, 10, 11)),
]
N_KEYS = 12                                   # + 1 key that no trace touches


def lim_keys(lid):
    return rl_amd.mix64(np.arange(N_KEYS + 1, dtype=np.uint64) + np.uint64((lid + 1) << 32))


def lim_trace(lid):
    """Limiter lid's trace: keys Pareto(1.1)-skewed over its 12 keys, evenly spaced times."""
    _, n, span, pmax, _ = CASES[lid]
    rng = np.random.default_rng(1000 + lid)
    ranks = np.minimum(rng.pareto(1.1, n).astype(np.int64), N_KEYS - 1)
    keys = lim_keys(lid)[ranks]
    permits = rng.integers(1, pmax + 1, n).astype(np.int32)
    now = (T0 * NS + (np.arange(n, dtype=np.int64) * span * NS) // n).astype(np.int64)
    return keys, permits, now, np.full(n, lid, np.uint16)


def trace_end(lid):
    return T0 + CASES[lid][2]


def new_oracle():
    o = PyOracle()
    for (algo, mx, w, rate, ttl), *_ in CASES:
        o.add_limiter(algo, mx, w, rate, local_cache_ttl_ms=ttl)
    for lid in range(len(CASES)):
        o.run(*lim_trace(lid))
    return o


def new_engine(**kw):
    e = rl_amd.Engine(max_batch=1 << 16, capacity=1 << 10, **kw)
    for (algo, mx, w, rate, ttl), *_ in CASES:
        e.add_limiter(algo, mx, w, rate, local_cache_ttl_ms=ttl)
    return e


def feed(e):
    for lid in range(len(CASES)):
        a, r, _, st = e.execute(*lim_trace(lid), want_tokens=False)
        assert st == rl_amd.RL_OK
    return e


def scan_waits(o, lid, key, permits, now):
    """The definition for one (limiter, key, now) and several permits: per candidate t a copy
    of the key's part of the oracle takes one acquire. Full scan; no denial after an allow."""
    L = o.limiters[lid]
    pre = (f"{lid}|rl:{key}:", f"{lid}|tb:{key}")
    kv = {k: v for k, v in o.redis.kv.items() if k.startswith(pre[0]) or k == pre[1]}
    exp = {k: o.redis.exp[k] for k in kv if k in o.redis.exp}
    cache = {k: v for k, v in o.cache.items() if k == (lid, key)}
    m = PyOracle()
    m.limiters = o.limiters
    first = {p: None for p in permits}
    for t in range(now, now + 2 * L.window_ms + L.cache_ttl + 2 + 1):
        for p in permits:
            m.redis.kv, m.redis.exp, m.cache = dict(kv), dict(exp), dict(cache)   # the copy
            ok = (m._sw_acquire(L, key, p, t) if L.algo == rl_amd.SW else m._tb_acquire(L, key, p, t))[0]
            if ok and first[p] is None:
                first[p] = t
            assert ok or first[p] is None, ("a denial after the first allow", lid, key, p, now, t)
    out = []
    for p in permits:
        if p > L.max_permits:
            assert first[p] is None
            out.append(NEVER)
        else:
            assert first[p] is not None, ("no allow inside the bound", lid, key, p, now)
            out.append(first[p] - now)
    return out


def query_set(lid):
    """13 keys x the limiter's query permits at the trace end and at end + 1, + 37, + w."""
    w, qp = CASES[lid][0][2], CASES[lid][4]
    keys = lim_keys(lid)
    k, p, t = [], [], []
    for dt in (0, 1, 37, w):
        for key in keys:
            for pp in qp:
                k.append(key); p.append(pp); t.append((trace_end(lid) + dt) * NS)
    return (np.array(k, np.uint64), np.array(p, np.int32), np.array(t, np.int64),
            np.full(len(k), lid, np.uint16))


@pytest.fixture(scope="module")
def oracle():
    return new_oracle()


@pytest.fixture(scope="module")
def reference(oracle):
    """Per limiter: its query set and the expected waits (computed once, never changed)."""
    ref = []
    for lid in range(len(CASES)):
        k, p, t, l = query_set(lid)
        want = np.zeros(len(k), np.int64)
        qp = CASES[lid][4]
        for i in range(0, len(k), len(qp)):
            want[i:i + len(qp)] = scan_waits(oracle, lid, int(k[i]), qp, int(t[i]) // NS)
        # the set must not pass vacuously (asserted on the oracle's answers alone)
        n = len(want)
        assert (want > 0).sum() >= 0.25 * n, (lid, (want > 0).sum(), n)
        assert (want == 0).sum() >= 0.10 * n, (lid, (want == 0).sum(), n)
        assert (want == NEVER).sum() > 0
        want.setflags(write=False)
        ref.append((k, p, t, l, want))
    return ref


@pytest.fixture(scope="module")
def fed_engine():
    """An engine after the five traces, for the tests that only query it."""
    e = feed(new_engine())
    yield e
    e.close()


def _mismatch(got, want, k, p, t):
    bad = np.nonzero(got != want)[0]
    return f"{bad.size} of {len(want)} differ, first: " + ", ".join(
        f"[{i}] key {int(k[i]):#x} p {p[i]} now {t[i] // NS}: got {got[i]} want {want[i]}" for i in bad[:5])


pytestmark = pytest.mark.gpu


# ---- 1. five small limiters
@pytest.mark.parametrize("lid", range(len(CASES)))
def test_each_limiter_equals_the_scan(fed_engine, reference, lid):
    k, p, t, l, want = reference[lid]
    got, st = fed_engine.retry_after(l, k, p, t)
    assert st == rl_amd.RL_OK
    assert np.array_equal(got, want), _mismatch(got, want, k, p, t)
    w, ttl = CASES[lid][0][2], CASES[lid][0][4]
    assert got.max() <= 2 * w + ttl + 1
    # a scalar limiter id and NULL skip / limiter take the same path as the arrays
    if lid == 0:
        wait = np.zeros(len(k), np.int64)
        st = fed_engine._L.rl_retry_after(fed_engine.handle, len(k), rl_amd._p(k), rl_amd._p(p),
                                          rl_amd._p(t), None, None, rl_amd._p(wait))
        assert st == rl_amd.RL_OK and np.array_equal(wait, want)


# ---- 2. one call mixing all five limiters, with invalid entries
def test_mixed_call_with_invalid_entries(fed_engine, reference):
    k = np.concatenate([r[0] for r in reference])
    p = np.concatenate([r[1] for r in reference])
    t = np.concatenate([r[2] for r in reference])
    l = np.concatenate([r[3] for r in reference])
    want = np.concatenate([r[4] for r in reference])
    perm = np.random.default_rng(5).permutation(len(k))
    k, p, t, l, want = k[perm], p[perm], t[perm], l[perm], want[perm]
    got, st = fed_engine.retry_after(l, k, p, t)
    assert st == rl_amd.RL_OK and np.array_equal(got, want), _mismatch(got, want, k, p, t)
    # permits 0, permits -3, limiter 99: -2 each, RL_E_INVALID_REQUEST, the rest unchanged
    at = [3, len(k) // 2, len(k) - 1]
    k2 = np.insert(k, at, k[at])
    t2 = np.insert(t, at, t[at])
    p2 = np.insert(p, at, [0, -3, 1])
    l2 = np.insert(l, at, [l[at[0]], l[at[1]], 99])
    bad = np.zeros(len(k2), bool)
    bad[[at[0], at[1] + 1, at[2] + 2]] = True
    assert list(p2[bad]) == [0, -3, 1] and l2[bad][2] == 99
    got2, st2 = fed_engine.retry_after(l2, k2, p2, t2)
    assert st2 == rl_amd.RL_E_INVALID_REQUEST
    assert np.all(got2[bad] == INVALID)
    assert np.array_equal(got2[~bad], want)
    # argument errors of the host entry
    L, h = fed_engine._L, fed_engine.handle
    w = np.zeros(4, np.int64)
    assert L.rl_retry_after(h, 4, None, rl_amd._p(p), rl_amd._p(t), None, None, rl_amd._p(w)) == rl_amd.RL_E_INVALID_ARG
    assert L.rl_retry_after(h, 4, rl_amd._p(k), rl_amd._p(p), rl_amd._p(t), None, None, None) == rl_amd.RL_E_INVALID_ARG
    assert L.rl_retry_after(h, (1 << 16) + 1, rl_amd._p(k), rl_amd._p(p), rl_amd._p(t), None, None,
                            rl_amd._p(w)) == rl_amd.RL_E_TOO_LARGE
    assert L.rl_retry_after(h, 0, None, None, None, None, None, None) == rl_amd.RL_OK


def _end_batch(dt=0):
    """One acquire per (limiter, key, query permits) at the limiter's trace end + dt."""
    k, p, t, l = [], [], [], []
    for lid in range(len(CASES)):
        for key in lim_keys(lid):
            for pp in CASES[lid][4][:3]:
                k.append(key); p.append(pp); t.append((trace_end(lid) + dt) * NS); l.append(lid)
    o = np.argsort(np.array(t), kind="stable")
    return (np.array(k, np.uint64)[o], np.array(p, np.int32)[o], np.array(t, np.int64)[o],
            np.array(l, np.uint16)[o])


# ---- 3. skip
def test_skip_takes_a_batchs_allowed():
    e = feed(new_engine())
    k, p, t, l = _end_batch()
    a, r, _, st = e.execute(k, p, t, l, want_tokens=False)
    assert st == rl_amd.RL_OK
    assert 0.1 * len(a) < a.sum() < 0.9 * len(a)
    plain, st1 = e.retry_after(l, k, p, t)
    skipped, st2 = e.retry_after(l, k, p, t, skip=a)
    assert st1 == rl_amd.RL_OK and st2 == rl_amd.RL_OK
    assert np.all(skipped[a != 0] == 0)
    assert np.array_equal(skipped[a == 0], plain[a == 0])
    assert (plain[a != 0] > 0).sum() > 0          # the skip did skip: those are not 0 by themselves
    assert (plain[a == 0] > 0).sum() > 0
    # a skipped entry is not looked at at all, invalid or not
    p2 = p.copy()
    p2[a != 0] = 0
    again, st3 = e.retry_after(l, k, p2, t, skip=a)
    assert st3 == rl_amd.RL_OK and np.array_equal(again, skipped)
    e.close()


# ---- 4. read-only
def test_queries_change_nothing(oracle, reference):
    e = feed(new_engine())
    at = max(trace_end(lid) for lid in range(len(CASES))) * NS
    order = ["limiter", "key_hash", "kind", "window_start_ms"]
    before = np.sort(e.export_state(at), order=order)
    stats0, status0 = e.stats(), e.last_status()
    for k, p, t, l, want in reference:
        got, _ = e.retry_after(l, k, p, t)
        assert np.array_equal(got, want)
    assert e.stats() == stats0 and e.last_status() == status0
    after = np.sort(e.export_state(at), order=order)
    assert before.size > 0 and np.array_equal(before, after)
    # the next batch still matches the oracle, the cache-on limiter's cache hits included
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


# ---- 5. probing, tombstones, growth
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
    got, st = e.retry_after(0, qk, qp, qt)
    assert st == rl_amd.RL_OK
    assert np.array_equal(got == NEVER, qp > 5)
    fin = got >= 0
    assert (got[fin] > 0).sum() > 400 and (got[fin] == 0).sum() > 400
    assert got.max() <= 2 * 1000 + 1
    # the bracket: peeks (remaining = (long) balance) at now + r - 1 and now + r, in time order
    now_ms = qt // NS
    idx = np.nonzero(fin)[0]
    pk = np.concatenate([qk[idx], qk[idx]])
    pt = np.concatenate([now_ms[idx] + got[idx] - 1, now_ms[idx] + got[idx]]) * NS
    side = np.concatenate([np.zeros(len(idx), bool), np.ones(len(idx), bool)])
    need = np.concatenate([qp[idx], qp[idx]]).astype(np.int64)
    first_ms = np.concatenate([got[idx] == 0, np.zeros(len(idx), bool)])   # r = 0: no t - 1 to refute
    od = np.argsort(pt, kind="stable")
    _, rem, _, _ = o.run(pk[od], np.ones(len(od), np.int32), pt[od].astype(np.int64),
                         ops=np.full(len(od), rl_amd.OP_PEEK, np.uint8), want_tokens=False)
    ok = np.where(side[od], rem >= need[od], (rem < need[od]) | first_ms[od])
    assert ok.all(), f"{(~ok).sum()} bracket failures"
    e.close()
    o.close()


# ---- 6. device entry
def test_device_entry_equals_host_entry(fed_engine, reference):
    import torch
    k = np.concatenate([r[0] for r in reference])
    p = np.concatenate([r[1] for r in reference])
    t = np.concatenate([r[2] for r in reference])
    l = np.concatenate([r[3] for r in reference])
    want = np.concatenate([r[4] for r in reference])
    skip = (np.arange(len(k)) % 3 == 0).astype(np.uint8)
    host, _ = fed_engine.retry_after(l, k, p, t, skip=skip)
    assert np.array_equal(host[skip == 0], want[skip == 0]) and np.all(host[skip != 0] == 0)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda()
           for x in (k.view(np.int64), p, t, l.view(np.int16), skip)]
    n = len(k)
    w1 = torch.full((n,), 77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    fed_engine.retry_after_device(n, *dev, w1)
    fed_engine.sync()
    assert np.array_equal(w1.cpu().numpy(), host)
    # on a caller's stream: ordered behind its work, and its later work behind the query
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        w2 = torch.full((n,), 77, dtype=torch.int64, device="cuda")
        fed_engine.retry_after_device(n, dev[0], dev[1], dev[2], dev[3], None, w2, stream=s.cuda_stream)
        out = w2.clone()
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert fed_engine.last_status() == rl_amd.RL_OK


def test_device_query_is_ordered_behind_a_pipelined_batch(reference):
    """RL_OPT_PIPELINE: a query enqueued right after a device batch sees that batch."""
    import torch
    e = new_engine(pipeline=True)
    for lid in range(len(CASES)):
        k, p, t, l = lim_trace(lid)
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda()
               for x in (k.view(np.int64), p, t, l.view(np.int16))]
        a = torch.empty(len(k), dtype=torch.uint8, device="cuda")
        r = torch.empty(len(k), dtype=torch.int64, device="cuda")
        qk, qp, qt, ql, want = reference[lid]
        q = [torch.from_numpy(np.ascontiguousarray(x)).cuda()
             for x in (qk.view(np.int64), qp, qt, ql.view(np.int16))]
        w = torch.empty(len(qk), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        e.execute_device(len(k), *dev, None, a, r)
        e.retry_after_device(len(qk), *q, None, w)
        assert e.last_status() == rl_amd.RL_OK
        assert np.array_equal(w.cpu().numpy(), want), lid
    e.close()


# ---- 7. end to end
def test_acquire_is_denied_one_ms_before_and_allowed_at_the_wait(oracle, reference):
    picks, seen = [], set()
    for lid, (k, p, t, l, want) in enumerate(reference):
        for i in np.nonzero(want > 0)[0]:
            if (lid, int(k[i])) in seen:
                continue
            # on the oracle: denied at now + wait - 1, then allowed at now + wait (with the local
            # cache a denial may itself set a rejecting entry; such a pair is not a test of P)
            o = copy.deepcopy(oracle)
            at = int(t[i]) // NS + int(want[i])
            wa, _, _ = o.run([k[i]] * 2, [p[i]] * 2, [(at - 1) * NS, at * NS], [lid] * 2)
            if list(wa) == [0, 1]:
                seen.add((lid, int(k[i])))
                picks.append((int(k[i]), int(p[i]), at, lid))
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
