"""The three implementations of the sliding window's fraction (rl_device.hpp sw_pct: one
multiply, multiply + fma correction, true division; chosen per limiter by rl_engine.cpp
pct_flags) through every kernel path that consumes it, bit-exact against the CPU oracle.

The traces come from tests/window_cases.py: per window, keys filled to a chosen count and probed
in the next windows at the remainders where the fraction's last bit decides the estimate (the
CPU test tests/test_window_cases_model.py proves that a bare multiply would change at least 16
answers of every fma-class and divide-class trace), dense same-key runs over a window boundary,
background keys; and the same from timestamp 0, where Java's truncating division makes
prev_start == curr_start in the first window. Each path is forced at this small size with the
engine's knobs and, where a counter exists, asserted to have run. Every case runs in three or
more batches, so state crosses batches (and the largest window's batches stay inside the
compact record's time span)."""
import functools

import numpy as np
import pytest

import rl_amd
import window_cases as wc
from oracle.coracle import COracle
from oracle.rl_oracle import PyOracle
from test_gpu_parity import NS, assert_same

pytestmark = pytest.mark.gpu

CASES = [(w, epoch) for w in wc.WINDOWS for epoch in (False, True)]
IDS = [f"{wc.window_class(w)}-{w}-{'epoch' if e else 't0'}" for w, e in CASES]
EVERY = 1 << 30                                    # sparse_max: every region sparse
cases = pytest.mark.parametrize("w,epoch", CASES, ids=IDS)


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(w, epoch, cache_ttl=0):
    """A window's limiters, trace, batch cuts and the oracle's answer (computed once, read-only)."""
    lims = wc.limiters(w, cache_ttl)
    tr = frozen(*wc.window_trace(w, epoch))
    o = COracle(lims)
    want = frozen(*o.run(*tr)[:3])
    return lims, tr, wc.batch_cuts(tr, 3), want, o.cache_hits()


def run(lims, tr, cuts, tune=None, want_status=(rl_amd.RL_OK,), **kw):
    """The trace through one engine, batch by batch (the run() of test_gpu_hot.py with explicit
    cuts); returns the results, the engine and the per-batch stats."""
    kw.setdefault("max_batch", 1 << 16)
    kw.setdefault("capacity", 1 << 14)
    e = rl_amd.Engine(**kw)
    for l in lims:
        e.add_limiter(*l)
    for k, v in (tune or {}).items():
        e.tune(k, v)
    got, stats = [[], [], []], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        ga, gr, gt, st = e.execute(*(x[a:b] for x in tr))
        assert st in want_status, rl_amd.strerror(st)
        got[0].append(ga); got[1].append(gr); got[2].append(gt)
        stats.append(e.stats())
    return tuple(np.concatenate(g) for g in got), e, stats


# ---------------------------------------------------------------- region scan, image mode
@cases
def test_region_scan(w, epoch):
    lims, tr, cuts, want, _ = case(w, epoch)
    got, e, _ = run(lims, tr, cuts)
    assert_same(got, want, f"regions w={w}")
    e.close()


@pytest.mark.parametrize("w", wc.DIV_WINDOWS)
def test_region_scan_wide_records(w):
    lims, tr, cuts, want, _ = case(w, False)
    got, e, _ = run(lims, tr, cuts, tune={"wide_records": 1})
    assert_same(got, want, f"wide records w={w}")
    e.close()


# ---------------------------------------------------------------- sparse regions
@cases
def test_sparse_regions(w, epoch):
    lims, tr, cuts, want, _ = case(w, epoch)
    sparse, e1, _ = run(lims, tr, cuts, tune={"sparse_max": EVERY})
    image, e0, _ = run(lims, tr, cuts, tune={"sparse_max": 0})
    assert_same(sparse, want, f"sparse w={w}")
    assert_same(image, want, f"image w={w}")
    assert_same(sparse, image, f"sparse vs image w={w}")
    e1.close(); e0.close()


# ---------------------------------------------------------------- cache-on rounds, solo
@pytest.mark.parametrize("ttl", [1, 50])
@cases
def test_cache_on_rounds(w, epoch, ttl):
    lims, tr, cuts, want, hits = case(w, epoch, ttl)
    got, e, stats = run(lims, tr, cuts, tune={"solo_threshold": 0})
    assert_same(got, want, f"cache ttl={ttl} w={w}")
    assert hits > 0                                             # the input reaches the cache
    assert sum(s["cache_hits"] for s in stats) == hits
    e.close()


@cases
def test_solo(w, epoch):
    lims, tr, cuts, want, hits = case(w, epoch, 50)
    for thr in (64, 0):
        got, e, stats = run(lims, tr, cuts, tune={"solo_threshold": thr})
        assert_same(got, want, f"solo_threshold={thr} w={w}")
        assert sum(s["cache_hits"] for s in stats) == hits
        e.close()


# ---------------------------------------------------------------- hot chains
@pytest.mark.parametrize("thr,split", [(1, 1), (1, 0), (256, 1), (256, 0)])
@cases
def test_hot_chains(w, epoch, thr, split):
    lims, tr, cuts, want, _ = case(w, epoch)
    got, e, stats = run(lims, tr, cuts, tune={"hot_threshold": thr, "chain_split": split})
    assert_same(got, want, f"hot_threshold={thr} chain_split={split} w={w}")
    assert max(s["hot_regions"] for s in stats) > 0, stats
    e.close()


# ---------------------------------------------------------------- allow walks
@pytest.mark.parametrize("w", list(wc.WALK_CASES),
                         ids=[f"{wc.window_class(w)}-{w}" for w in wc.WALK_CASES])
def test_allow_walks(w):
    """As test_gpu_walk.py's helper: walk on and off give the oracle's answer, and the last
    batch's per-region debug words (word 20 = walked allows) show whether the walk ran."""
    lims, tr, cuts = wc.walk_trace(w)
    want = COracle(lims).run(*tr)
    for walk in (1, 0):
        got, e, stats = run(lims, tr, cuts, capacity=1 << 12,
                            tune={"walk": walk, "walk_min": 0, "debug_regions": 1, "hot_threshold": 4096})
        assert_same(got, want, f"walk={walk} w={w}")
        walked = int(e.debug_region_times(1 << 16)[:, 20].sum())
        if walk:
            assert stats[-1]["hot_regions"] > 0
            assert walked > 0, "the walk did not run"
        else:
            assert walked == 0, f"walk=0: {walked} walked allows"
        e.close()


# ---------------------------------------------------------------- two-pass partition, routing
@cases
def test_two_pass_routed(w, epoch):
    lims, tr, cuts, want, _ = case(w, epoch)
    got, e, stats = run(lims, tr, cuts, capacity=1 << 22, tune={"route": 1, "hot_threshold": 256})
    assert_same(got, want, f"two-pass routed w={w}")
    assert sum(s["routed"] for s in stats[1:]) > 0, stats     # from the second batch on
    e.close()


# ---------------------------------------------------------------- retry-after
def near_epoch_instant(w):
    """Late in the first window of an epoch trace (0 <= now < w, where the current bucket is read
    twice and the fill keys come up against max): the waits from here run into the second window."""
    return w - max(w // 8, 1)


def retry_setup(w, epoch, tq=None):
    """The trace up to the instant tq (default: a third of its third window), run on an engine in
    three batches; the queries at tq: the "limit" keys with 1 .. 48 permits (their answers are the
    successive instants at which the estimate falls by one), every other fill key and the dense
    runs' keys with 1 and 3."""
    lims, tr, _, _, _ = case(w, epoch)
    if tq is None:
        tq = wc.start_ms(w, epoch) + 2 * w + w // 3
    n = int(np.searchsorted(tr[2], tq * NS, side="left"))
    pre = tuple(x[:n] for x in tr)
    got, e, _ = run(lims, pre, wc.batch_cuts(pre, 3))
    qk, qp, ql = [], [], []
    for i, (lim, _, mode) in enumerate(wc.FILLS):
        for p in (range(1, 49) if mode == "limit" else (1, 3)):
            if p <= lims[lim][1]:
                qk.append(wc.fill_key(i)); qp.append(p); ql.append(lim)
    for i, lim in ((100, 1), (101, 2)):
        for p in (1, 3):
            qk.append(wc.fill_key(i)); qp.append(p); ql.append(lim)
    return (lims, pre, got, e, tq, np.array(qk, np.uint64), np.array(qp, np.int32),
            np.array(ql, np.uint16))


@pytest.mark.parametrize("w,epoch", [c for c in CASES if c[0] <= 1024],
                         ids=[i for c, i in zip(CASES, IDS) if c[0] <= 1024])
def test_retry_after_equals_the_scan(w, epoch):
    """Windows up to 1024 ms: the full scan of test_gpu_retry_after.py on the Python oracle."""
    check_retry_scan(w, epoch)


@pytest.mark.parametrize("w", [w for w in wc.WINDOWS if w <= 1024],
                         ids=[f"{wc.window_class(w)}-{w}" for w in wc.WINDOWS if w <= 1024])
def test_retry_after_equals_the_scan_near_epoch(w):
    """The same with 0 <= now < w: queries inside the first window of the epoch trace."""
    check_retry_scan(w, True, near_epoch_instant(w))


def check_retry_scan(w, epoch, tq=None):
    from test_gpu_retry_after import scan_waits
    lims, pre, got, e, tq, qk, qp, ql = retry_setup(w, epoch, tq)
    o = PyOracle()
    for l in lims:
        o.add_limiter(*l)
    wa, wr, _ = o.run(*pre)
    assert_same(got, (wa, wr, None), f"prefix w={w}")
    wait, st = e.retry_after(ql, qk, qp, np.full(len(qk), tq * NS, np.int64))
    assert st == rl_amd.RL_OK
    want = np.zeros(len(qk), np.int64)
    for key, lim in sorted({(int(k), int(l)) for k, l in zip(qk, ql)}):
        m = (qk == np.uint64(key)) & (ql == lim)
        want[m] = scan_waits(o, lim, key, tuple(int(p) for p in qp[m]), tq)
    assert (want > 0).sum() >= 8 and (want == 0).sum() >= 1, want
    assert np.array_equal(wait, want), list(zip(qk[wait != want], qp[wait != want],
                                                wait[wait != want], want[wait != want]))[:5]
    e.close()


@pytest.mark.parametrize("w,epoch", [c for c in CASES if c[0] > 1024],
                         ids=[i for c, i in zip(CASES, IDS) if c[0] > 1024])
def test_retry_after_brackets(w, epoch):
    """Larger windows: wait == 0 exactly when the oracle allows at now; at now + wait the oracle
    has room for the permits and at now + wait - 1 it has not (peeks: for a sliding window
    without the local cache an acquire of p is allowed exactly when a peek reads >= p), and for
    one query per key the acquires themselves: denied at now + wait - 1, allowed at now + wait,
    on the oracle and on the engine."""
    check_retry_brackets(w, epoch)


@pytest.mark.parametrize("w", [w for w in wc.WINDOWS if w > 1024],
                         ids=[f"{wc.window_class(w)}-{w}" for w in wc.WINDOWS if w > 1024])
def test_retry_after_brackets_near_epoch(w):
    """The same with 0 <= now < w: queries inside the first window of the epoch trace."""
    check_retry_brackets(w, True, near_epoch_instant(w))


def check_retry_brackets(w, epoch, tq=None):
    lims, pre, got, e, tq, qk, qp, ql = retry_setup(w, epoch, tq)
    o = COracle(lims)
    assert_same(got, o.run(*pre)[:3], f"prefix w={w}")
    n = len(qk)
    wait, st = e.retry_after(ql, qk, qp, np.full(n, tq * NS, np.int64))
    assert st == rl_amd.RL_OK and (wait >= 0).all()
    peek = np.full(n, wc.OP_PEEK, np.uint8)
    ones = np.ones(n, np.int32)
    at_now = o.run(qk, ones, np.full(n, tq * NS, np.int64), ql, peek)[1]
    assert np.array_equal(wait == 0, at_now >= qp)
    at_wait = o.run(qk, ones, (tq + wait) * NS, ql, peek)[1]
    before = o.run(qk, ones, (tq + wait - 1) * NS, ql, peek)[1]
    assert (at_wait >= qp).all()
    assert ((before < qp) | (wait == 0)).all()
    assert (wait > 0).sum() >= 8 and (wait == 0).sum() >= 1, wait
    # the acquires, one positive-wait query per key (a denied acquire changes nothing)
    first = {}
    for i in np.nonzero(wait > 0)[0]:
        first.setdefault((int(qk[i]), int(ql[i])), i)
    idx = np.array(sorted(first.values()))
    k = np.repeat(qk[idx], 2); p = np.repeat(qp[idx], 2); l = np.repeat(ql[idx], 2)
    t = np.stack([tq + wait[idx] - 1, tq + wait[idx]], 1).ravel() * NS
    od = np.argsort(t, kind="stable")
    pair = (k[od], p[od], t[od], l[od], np.zeros(len(od), np.uint8))
    wa = o.run(*pair)[0]
    ga = e.execute(*pair)[0]
    back = np.empty_like(wa); back[od] = wa
    assert np.array_equal(back, np.tile(np.array([0, 1], np.uint8), len(idx)))
    assert np.array_equal(ga, wa)
    e.close()


# ---------------------------------------------------------------- peek and census
@cases
def test_peek_and_census(w, epoch):
    """After the fill window alone (two batches): rl_available of every key at the instants of
    the next window where the multiply is wrong for the fill counts (any point for the multiply
    class), and the census (used = max - available, summed; the exhausted keys; the heaviest
    consumers) at three of them, against the oracle's peeks."""
    lims, tr, _, _, _ = case(w, epoch)
    pre, w1 = wc.fill_prefix(tr, w, epoch)
    got, e, _ = run(lims, pre, wc.batch_cuts(pre, 2))
    o = COracle(lims)
    assert_same(got, o.run(*pre)[:3], f"fill window w={w}")
    rs = set()
    for lim, P, _ in wc.FILLS:
        P = wc.fill_count(P, w)
        r = wc.mul_wrong(w, P)
        rs.update((r if len(r) else wc.points(w, P))[:16].tolist())
    rs = sorted(rs)[:48]
    assert len(rs) >= 3
    check_census(e, o, lims, pre, [w1 + r for r in rs])
    e.close()


@pytest.mark.parametrize("w", wc.WINDOWS, ids=[f"{wc.window_class(w)}-{w}" for w in wc.WINDOWS])
def test_peek_and_census_near_epoch(w):
    """The same with 0 <= now < w: the epoch trace up to a point of its first window, then
    rl_available and the census at instants of the rest of that window, where prev_start ==
    curr_start and the current bucket counts twice."""
    lims, tr, _, _, _ = case(w, True)
    pre, instants = near_epoch_census_inputs(w)
    got, e, _ = run(lims, pre, wc.batch_cuts(pre, 2))
    o = COracle(lims)
    assert_same(got, o.run(*pre)[:3], f"part of the fill window w={w}")
    used = check_census(e, o, lims, pre, instants)
    assert used > 0
    e.close()


def near_epoch_census_inputs(w):
    """The epoch trace up to the request that brings the third fill key (peeks only, max 1000) to
    c = fill_count(250, w) allowed requests, and up to 12 later instants of the first window.
    There the estimate is d2l(c * (1 - r / w) + c), so the instants are taken where c * (w - r) / w
    is an integer, first of all where the bare multiply gets that estimate wrong, and filled up
    with evenly spaced ones. (Such instants are rare: the bucket counted twice puts the sum at
    least a binade above the weighted part, whose last bit then shows only on a rounding tie. The
    row is about the prev_start == curr_start branch of the query kernels.)"""
    lims, tr, _, _, _ = case(w, True)
    c = wc.fill_count(250, w)
    mine = np.nonzero((tr[0] == np.uint64(wc.fill_key(2))) & (tr[4] == wc.OP_ACQUIRE))[0]
    n = int(mine[c - 1]) + 1
    pre = tuple(x[:n] for x in tr)
    cut = int(pre[2][-1] // NS)
    assert cut < w - 1 and COracle(lims).run(*pre)[0][mine[:c]].all()      # c allowed, now < w
    r = wc.points(w, c)
    r = r[r > cut]
    r = r if len(r) else np.arange(cut + 1, w)
    true, mul = wc.estimates(w, c, r, c)
    even = np.linspace(cut + 1, w - 1, 6).astype(np.int64)
    pick = np.concatenate([r[true != mul][:9], r[true == mul][:12]])[:12]
    return pre, np.unique(np.concatenate([pick, even])).tolist()


def check_census(e, o, lims, pre, instants):
    """rl_available of every key of the trace at every instant, the census at three of them;
    returns the used permits it saw."""
    total = 0
    for lid in range(len(lims)):
        keys = np.unique(pre[0][pre[3] == lid])
        mx = lims[lid][1]
        for j, at in enumerate(instants):
            now = np.full(len(keys), at * NS, np.int64)
            avail, st = e.available(lid, keys, now)
            want = o.run(keys, np.ones(len(keys), np.int32), now, np.full(len(keys), lid, np.uint16),
                         np.full(len(keys), wc.OP_PEEK, np.uint8))[1]
            assert st == rl_amd.RL_OK and np.array_equal(avail, want), (lid, at)
            if j % (len(instants) // 3) == 0:
                used = mx - np.clip(want, 0, mx)
                total += int(used.sum())
                u = e.limiter_usage(lid, at * NS)
                assert u["used_permits"] == int(used.sum()), (lid, at)
                assert u["exhausted_keys"] == int((used == mx).sum()), (lid, at)
                m = used >= 1
                order = np.lexsort((keys[m], -used[m]))
                gk, gu, n_match = e.top_consumers(lid, at * NS, 64, 1)
                assert n_match == int(m.sum())
                np.testing.assert_array_equal(gk, keys[m][order][:64])
                np.testing.assert_array_equal(gu, used[m][order][:64])
    return total


# ---------------------------------------------------------------- seeded state, large counts
@pytest.mark.parametrize("w", [1024, 1000, 4_200_000],
                         ids=[f"{wc.window_class(w)}-{w}" for w in (1024, 1000, 4_200_000)])
def test_seeded_large_counts(w):
    """d2l(prev * weight + (curr + k)) where the sum is near 2^31: 36 keys imported with a
    previous bucket of P and a current bucket of C0 under max_permits 2^31 - 2 (wide records),
    C0 chosen so that the estimate at the key's first probe is max - d for d = 0, 1, 2, 3, 5, 20;
    then ~1000 acquires and peeks at remainders where P * (w - r) / w is an integer, against the
    Python oracle loaded with the same keyspace. At these counts the sum's own rounding hides the
    fraction's last bit unless prev * weight lies in the sum's binade, so the first probe is, where
    one exists, a remainder at which the bare multiply gives another estimate at exactly that C0."""
    mx = (1 << 31) - 2
    lim = (rl_amd.SW, mx, w, 0.0)
    e = rl_amd.Engine(max_batch=1 << 12, capacity=1 << 10)
    e.add_limiter(*lim)
    assert e.result_width() == 8
    o = PyOracle()
    o.add_limiter(*lim)
    w1 = wc.start_ms(w, False) + w
    rng = np.random.default_rng(w)
    p_list = (mx // w * w, 2_000_000_000 // w * w, 1 << 30, 3 << 29, mx, mx - 1)
    pts = {}
    for P in p_list:
        r = wc.points(w, P)
        pts[P] = r if len(r) else np.arange(1, w, max(w // 4096, 1))     # (none: any remainders)
    seeds, n_wrong = [], 0                          # (key, P, C0, probe remainders)
    for i in range(36):
        P, d = p_list[i % 6], (0, 1, 2, 3, 5, 20)[i // 6]
        r = pts[P]
        true, mul = wc.estimates(w, P, r, mx - P * (w - r) // w - d)
        bad = r[true != mul]
        n_wrong += len(bad) > 0
        r0 = int(rng.choice(bad if len(bad) else r))
        after = r[r >= r0]
        probes = np.unique(np.concatenate([[r0], rng.choice(after, min(len(after), 6), replace=False)]))
        seeds.append((wc.fill_key(300 + i), P, max(mx - P * (w - r0) // w - d, 1), probes))
    assert wc.window_class(w) == "mul" or n_wrong >= 6, n_wrong
    ent = np.zeros(2 * len(seeds), rl_amd.STATE_DTYPE)
    space = []
    for i, (key, P, c0, _) in enumerate(seeds):
        for j, (start, count, exp) in enumerate(((w1 - w, P, w1 + w - 1), (w1, c0, w1 + w))):
            x = ent[2 * i + j]
            x["key_hash"], x["limiter"], x["kind"] = key, 0, rl_amd.STATE_SW_BUCKET
            x["window_start_ms"], x["count"], x["expire_at_ms"] = start, count, exp
            space.append((0, key, 0, start, count, 0.0, 0, exp))
    assert e.import_state(ent) == (rl_amd.RL_OK, len(ent))
    o.load_keyspace(space)
    k, p, t, op = [], [], [], []
    for key, P, c0, r in seeds:
        for rr in r.tolist():
            k += [key] * 4; t += [w1 + rr] * 4
            p += [1, 2, 1, 1]; op += [0, 0, 1, 0]
    od = np.argsort(np.array(t), kind="stable")
    req = (np.array(k, np.uint64)[od], np.array(p, np.int32)[od], np.array(t, np.int64)[od] * NS,
           np.zeros(len(od), np.uint16), np.array(op, np.uint8)[od])
    wa, wr, _ = o.run(*req)
    wa, wr = np.array(wa, np.uint8), np.array(wr, np.int64)
    assert 0 < wa.sum() < (req[4] == 0).sum() and (wr == 0).any() and (wr > 0).any()
    n = len(od)
    got_a, got_r = [], []
    for a, b in ((0, n // 2), (n // 2, n)):
        ga, gr, _, st = e.execute(*(x[a:b] for x in req))
        assert st == rl_amd.RL_OK
        got_a.append(ga); got_r.append(gr)
    assert_same((np.concatenate(got_a), np.concatenate(got_r), None), (wa, wr, None), f"seeded w={w}")
    e.close()
