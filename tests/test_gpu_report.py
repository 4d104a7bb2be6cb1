"""rl_tally_batch / rl_top_denied on the GPU: exact equality, in every field of every row and in
every returned key and count, with the definition restated in numpy (tests/report_cases.py)."""
import ctypes

import numpy as np
import pytest

import report_cases as rc
import rl_amd
import test_gpu_retry_after as ra
from oracle.rl_oracle import PyOracle

pytestmark = pytest.mark.gpu

MAX_BATCH = 4096
N_HOST = 3 * MAX_BATCH + 5                     # three full pieces and a ragged one
TALLY_N = (0, 1, 63, 64, 65, 2047, 2048, 2049, 10257)
FIELDS = rl_amd.TALLY_DTYPE.names


def dev(x):
    import torch
    if x is None:
        return None
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint16:
        x = x.view(np.int16)
    elif x.dtype == np.uint64:
        x = x.view(np.int64)
    t = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()                   # the engine's stream is not torch's: the copy is done
    return t


def new_out(fill=0):
    import torch
    out = torch.full((rl_amd.TALLY_ROWS * 12,), fill, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                   # (the fill too, before the engine's stream writes)
    return out


def rows_of(out):
    return out.cpu().numpy().view(rl_amd.TALLY_DTYPE)


def diff(got, want):
    bad = [(r, f, int(got[f][r]), int(want[f][r])) for f in FIELDS[:10] for r in range(rl_amd.TALLY_ROWS)
           if got[f][r] != want[f][r]]
    return f"{len(bad)} cells differ (row, field, got, want): {bad[:6]}"


def same(got, want):
    return got.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def engines():
    """One small engine per limiter mix: only its limiter count enters the report."""
    es = {}
    for mix in rc.MIXES:
        e = rl_amd.Engine(max_batch=MAX_BATCH, capacity=256)
        for _ in range(rc.MIX_LIMITERS[mix]):
            e.add_limiter(rl_amd.SW, 10, 1000)
        es[mix] = e
    yield es
    for e in es.values():
        e.close()


# ---- 1. the tally on synthetic arrays
@pytest.mark.parametrize("mix", rc.MIXES)
def test_tally_equals_the_definition(engines, mix):
    e = engines[mix]
    for n in TALLY_N:
        n_lim, p, lim, op, al, rem = rc.synth(n, mix)
        d = [dev(x) for x in (p, lim, op, al, rem)]
        for use_lim, use_op in ((True, True), (False, True), (True, False), (False, False)):
            want = rc.tally_model(n_lim, p, lim if use_lim else None, op if use_op else None, al, rem)
            out = new_out(-1)                                   # 0xFF everywhere: fully overwritten
            e.tally_batch_device(n, d[0], d[1] if use_lim else None, d[2] if use_op else None, d[3], d[4], out)
            e.sync()
            got = rows_of(out)
            assert same(got, want), (mix, n, use_lim, use_op, diff(got, want))
        # what the inputs must contain for the case to mean something (asserted on the model)
        want = rc.tally_model(n_lim, p, lim, op, al, rem)
        assert np.all(want["requests"] == want["invalid"] + want["errors"] + want["allowed"] +
                      want["denied"] + want["peeks"] + want["resets"])
        if n == 10257:
            assert all(int(want[f].sum()) > 0 for f in FIELDS[:10]), mix
            assert int(want["permits_allowed"].max()) > 1 << 32
            assert {0, 1, 2, 3, 255} <= set(op.tolist()) and {-1, -2, -3, 0, 5} <= set(rem.tolist())
            if mix == "wide":
                assert int((want["requests"] > 0).sum()) == 255        # 254 limiters and row 255
                assert any(len(set(lim[w:w + 64].tolist())) == 64 for w in range(0, n - 64, 64))
                assert int(lim.max()) == 65535 and int(want["requests"][255]) > 64


def test_accumulate_adds_and_a_plain_call_overwrites(engines):
    e = engines["blocks10"]
    out = new_out(0)
    want = np.zeros(rl_amd.TALLY_ROWS, rl_amd.TALLY_DTYPE)
    for seed, n in ((1, 2049), (2, 65), (3, 10257)):
        n_lim, p, lim, op, al, rem = rc.synth(n, "blocks10", seed)
        want = rc.tally_model(n_lim, p, lim, op, al, rem, into=want)
        e.tally_batch_device(n, *[dev(x) for x in (p, lim, op, al, rem)], out, accumulate=True)
    e.sync()
    got = rows_of(out)
    assert same(got, want), diff(got, want)
    # n == 0 with the flag leaves it alone; without it everything is zero
    e.tally_batch_device(0, None, None, None, None, None, out, accumulate=True)
    e.sync()
    assert same(rows_of(out), want)
    e.tally_batch_device(0, None, None, None, None, None, out)
    e.sync()
    assert not rows_of(out).view(np.uint64).any()


def test_device_forms_on_a_callers_stream(engines):
    """Ordered behind the caller's work on that stream, and the caller's later work behind them."""
    import torch
    e = engines["three"]
    n_lim, p, lim, op, al, rem = rc.synth(10257, "three", 5)
    keys = np.random.default_rng(4).integers(0, 50, 10257).astype(np.uint64)
    d = [dev(x) for x in (keys, p, lim, op, al, rem)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = torch.full((rl_amd.TALLY_ROWS * 12,), -1, dtype=torch.int64, device="cuda")
        e.tally_batch_device(10257, *d[1:], out, stream=s.cuda_stream)
        copy = out.clone()
        tk, tc, heavy, den = e.top_denied_device(10257, *d, 1, 8, 1, stream=s.cuda_stream)
    s.synchronize()
    assert same(rows_of(copy), rc.tally_model(n_lim, p, lim, op, al, rem))
    wk, wc, wh, wd = rc.top_denied_model(n_lim, keys, p, lim, op, al, rem, 1, 8, 1)
    assert (heavy, den) == (wh, wd) and np.array_equal(tk.cpu().numpy(), wk) and np.array_equal(tc.cpu().numpy(), wc)


def test_host_forms_stage_three_pieces_and_a_ragged_one(engines):
    e = engines["three"]
    n_lim, p, lim, op, al, rem = rc.synth(N_HOST, "three", 7)
    want = rc.tally_model(n_lim, p, lim, op, al, rem)
    got = e.tally_batch(p, lim, op, al, rem)
    assert same(got, want), diff(got, want)
    assert same(e.tally_batch(p, None, None, al, rem), rc.tally_model(n_lim, p, None, None, al, rem))
    twice = e.tally_batch(p, lim, op, al, rem, out=got.copy())
    assert same(twice, rc.tally_model(n_lim, p, lim, op, al, rem, into=want))
    keys = np.random.default_rng(3).integers(0, 40, N_HOST).astype(np.uint64)
    for sel in range(3):
        tk, tc, heavy, den = e.top_denied(keys, p, lim, op, al, rem, sel, 16, 2)
        wk, wc, wh, wd = rc.top_denied_model(n_lim, keys, p, lim, op, al, rem, sel, 16, 2)
        assert wd > 100 and wh > 16
        assert (heavy, den) == (wh, wd) and np.array_equal(tk, wk) and np.array_equal(tc, wc), sel


def test_argument_errors_with_a_live_engine(engines):
    e = engines["three"]
    L, h, p_ = e._L, e.handle, rl_amd._p
    n_lim, p, lim, op, al, rem = rc.synth(65, "three")
    d = [dev(x) for x in (p, lim, op, al, rem)]
    out = new_out(-1)
    bad = rl_amd.RL_E_INVALID_ARG
    dp = [p_(x) for x in d]
    assert L.rl_tally_batch_device(h, 65, dp[0], dp[1], dp[2], dp[3], dp[4], p_(out), 2, None) == bad
    assert L.rl_tally_batch_device(h, 65, dp[0], dp[1], dp[2], dp[3], dp[4], ctypes.c_void_p(out.data_ptr() + 4),
                                   0, None) == bad
    assert L.rl_tally_batch_device(h, 65, None, dp[1], dp[2], dp[3], dp[4], p_(out), 0, None) == bad
    assert L.rl_tally_batch_device(h, 65, dp[0], dp[1], dp[2], dp[3], dp[4], None, 0, None) == bad
    assert L.rl_tally_batch_device(h, (1 << 31) + 1, dp[0], dp[1], dp[2], dp[3], dp[4], p_(out), 0, None) == \
        rl_amd.RL_E_TOO_LARGE
    host_out = np.zeros(rl_amd.TALLY_ROWS, rl_amd.TALLY_DTYPE)
    assert L.rl_tally_batch(h, 65, p_(p), p_(lim), p_(op), p_(al), p_(rem), p_(host_out), 4) == bad
    e.sync()
    assert np.all(rows_of(out).view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF))
    keys = np.arange(65, dtype=np.uint64)
    with pytest.raises(rl_amd.RlError) as ei:
        e.top_denied(keys, p, lim, op, al, rem, 3, 4, 1)              # sel_limiter == L
    assert ei.value.status == bad
    with pytest.raises(rl_amd.RlError) as ei:
        e.top_denied_device(65, dev(keys), d[0], d[1], d[2], d[3], d[4], 65535, 4, 1)
    assert ei.value.status == bad


# ---- 2. a real batch: the five limiters of the retry-after tests in one stream
def real_stream():
    parts = [ra.lim_trace(lid) for lid in range(len(ra.CASES))]
    k, p, t, l = (np.concatenate([x[i] for x in parts]) for i in range(4))
    rng = np.random.default_rng(77)
    # 50 invalid requests (unknown limiter, permits 0) and token-bucket requests above the maximum
    xt = rng.choice(t, 50 + 60)
    xk = np.concatenate([rng.integers(1, 1 << 62, 50).astype(np.uint64),
                         ra.lim_keys(0)[rng.integers(0, ra.N_KEYS, 30)], ra.lim_keys(2)[rng.integers(0, ra.N_KEYS, 30)]])
    xp = np.concatenate([np.zeros(50, np.int32), np.full(30, 6, np.int32), np.full(30, 8, np.int32)])
    xl = np.concatenate([np.full(50, 99, np.uint16), np.zeros(30, np.uint16), np.full(30, 2, np.uint16)])
    k, p, t, l = np.concatenate([k, xk]), np.concatenate([p, xp]), np.concatenate([t, xt]), np.concatenate([l, xl])
    o = np.argsort(t, kind="stable")
    return k[o], p[o], t[o], l[o]


@pytest.fixture(scope="module")
def real():
    """The stream, the engine's answers, the oracle's answers and the engine (read-only after)."""
    k, p, t, l = real_stream()
    o = PyOracle()
    for (algo, mx, w, rate, ttl), *_ in ra.CASES:
        o.add_limiter(algo, mx, w, rate, local_cache_ttl_ms=ttl)
    wa, wr, _ = o.run(k, p, t, l)
    e = ra.new_engine()
    a, r, _, st = e.execute(k, p, t, l, want_tokens=False)
    assert st == rl_amd.RL_E_INVALID_REQUEST
    yield dict(k=k, p=p, t=t, l=l, a=a, r=r, wa=np.array(wa, np.uint8), wr=np.array(wr, np.int64), e=e)
    e.close()


def test_real_batch_tally_equals_the_oracles_and_the_batch_stats(real):
    e, p, l, a, r = real["e"], real["p"], real["l"], real["a"], real["r"]
    n_lim = len(ra.CASES)
    at = int(real["t"].max())
    before = ([e.limiter_digest(lid, at, 3) for lid in range(n_lim)], e.stats(), e.last_status())
    got = e.tally_batch(p, l, None, a, r)
    oracle_tally = rc.tally_model(n_lim, p, l, None, real["wa"], real["wr"])
    assert same(got, oracle_tally), diff(got, oracle_tally)
    out = new_out(-1)
    e.tally_batch_device(len(p), dev(p), dev(l), None, dev(a), dev(r), out)
    e.sync()
    assert same(rows_of(out), oracle_tally)
    st = before[1]
    assert int(got["allowed"].sum()) == st["allowed"] and int(got["invalid"].sum()) == st["invalid"] == 50
    assert int(got["invalid"][rl_amd.TALLY_UNKNOWN]) == 50 and int(got["errors"].sum()) == 0
    assert int(got["over_max"][0]) == 30 and int(got["over_max"][2]) == 30
    assert all(int(got["denied"][lid]) > 100 and int(got["allowed"][lid]) > 40 for lid in range(n_lim))
    for lid in range(n_lim):
        e.top_denied(real["k"], p, l, None, a, r, lid, 8, 1)
    after = ([e.limiter_digest(lid, at, 3) for lid in range(n_lim)], e.stats(), e.last_status())
    for (d0, t0), (d1, t1) in zip(before[0], after[0]):
        assert d0.tobytes() == d1.tobytes() and t0 == t1
    assert before[1:] == after[1:]


@pytest.mark.parametrize("sel", range(len(ra.CASES)))
def test_real_batch_top_denied_per_limiter(real, sel):
    e, k, p, l, a, r = (real[x] for x in "ekplar")
    n_lim = len(ra.CASES)
    for kk, mc in ((4096, 1), (3, 1), (5, 20)):
        wk, wc, wh, wd = rc.top_denied_model(n_lim, k, p, l, None, a, r, sel, kk, mc)
        tk, tc, heavy, den = e.top_denied(k, p, l, None, a, r, sel, kk, mc)
        assert (heavy, den) == (wh, wd) and np.array_equal(tk, wk) and np.array_equal(tc, wc), (kk, mc)
        dk, dc, dheavy, dden = e.top_denied_device(len(k), dev(k), dev(p), dev(l), None, dev(a), dev(r), sel, kk, mc)
        assert (dheavy, dden) == (wh, wd)
        assert np.array_equal(dk.cpu().numpy(), wk) and np.array_equal(dc.cpu().numpy(), wc)
    assert wd > 100
    # only this limiter's keys: the others' denials stay out
    mine = set(ra.lim_keys(sel).tolist())
    full = e.top_denied(k, p, l, None, a, r, sel, 4096, 1)[0]
    assert len(full) > 3 and set(full.tolist()) <= mine


# ---- 3. top-denied on synthetic arrays
HOT, PEEKED, OTHER = 777, 888, 999
ALL_ONES = 0xFFFFFFFFFFFFFFFF


def denied_case():
    """N_HOST requests under three limiters, shuffled. Limiter 0's denials: key ~0 60 times, key 0
    50 times, keys 1000..1019 seven times each (the ties), 1500 keys once or twice."""
    rng = np.random.default_rng(11)
    k, l, op, al = [], [], [], []

    def add(key, cnt, lim, o, a):
        k.extend([key] * cnt); l.extend([lim] * cnt); op.extend([o] * cnt); al.extend([a] * cnt)

    add(HOT, 3000, 0, 0, 1)                     # the most frequent key overall: never denied
    add(PEEKED, 1500, 0, 1, 0)                  # often peeked (allowed 0 there means nothing)
    add(OTHER, 800, 1, 0, 0)                    # denied under limiter 1 only
    add(OTHER, 40, 0, 0, 1)
    add(ALL_ONES, 60, 0, 0, 0)
    add(0, 50, 0, 0, 0)
    for key in range(1000, 1020):
        add(key, 7, 0, 0, 0)
    for key in range(5000, 6500):
        add(key, 1 + key % 2, 0, 0, 0)
    add(HOT, 25, 99, 0, 0)                      # "denied" under an unknown limiter: invalid
    rest = N_HOST - len(k)
    assert rest > 1000
    for key in rng.integers(10_000, 10_400, rest).tolist():
        add(key, 1, 2, 0, int(rng.integers(0, 2)))
    o = rng.permutation(N_HOST)
    k, l = np.array(k, np.uint64)[o], np.array(l, np.uint16)[o]
    op, al = np.array(op, np.uint8)[o], np.array(al, np.uint8)[o]
    return k, np.ones(N_HOST, np.int32), l, op, al, np.zeros(N_HOST, np.int64)


def test_top_denied_selects_only_the_denied_of_one_limiter(engines):
    e = engines["three"]
    k, p, l, op, al, r = denied_case()
    assert np.unique(k, return_counts=True)[1].max() == 3025 and (k == HOT).sum() == 3025
    d = [dev(x) for x in (k, p, l, op, al, r)]
    for n in (1, 2047, 2049, N_HOST):
        sl = [x[:n] for x in (k, p, l, op, al, r)]
        ds = [x[:n] for x in d]
        for sel in (0, 1, 2):
            for kk, mc in ((4096, 1), (10, 1), (12, 7), (5, 2), (4096, 61)):
                wk, wc, wh, wd = rc.top_denied_model(3, *sl, sel, kk, mc)
                tk, tc, heavy, den = e.top_denied_device(n, *ds, sel, kk, mc)
                assert (heavy, den) == (wh, wd), (n, sel, kk, mc)
                assert np.array_equal(tk.cpu().numpy(), wk) and np.array_equal(tc.cpu().numpy(), wc), (n, sel, kk, mc)
    # what the full case shows (on the model, which the engine equalled above)
    wk, wc, wh, wd = rc.top_denied_model(3, k, p, l, op, al, r, 0, 4096, 1)
    assert HOT not in wk and PEEKED not in wk and OTHER not in wk
    assert list(wk[:2]) == [ALL_ONES, 0] and list(wc[:2]) == [60, 50]
    assert wh == 2 + 20 + 1500 and wd == 60 + 50 + 140 + 1500 + 750
    wk12, wc12, wh12, _ = rc.top_denied_model(3, k, p, l, op, al, r, 0, 12, 7)
    assert wh12 == 22 > 12 and list(wc12[2:]) == [7] * 10 and list(wk12[2:]) == list(range(1000, 1010))
    assert list(rc.top_denied_model(3, k, p, l, op, al, r, 1, 4096, 1)[0]) == [OTHER]
    # the host form on the same arrays (three pieces and a ragged one), tails untouched
    L, h, p_ = e._L, e.handle, rl_amd._p
    top, cnt = np.full(40, 7, np.uint64), np.full(40, 7, np.uint64)
    n_out, heavy, den = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    st = L.rl_top_denied(h, N_HOST, p_(k), p_(p), p_(l), p_(op), p_(al), p_(r), 0, 40, 7, p_(top), p_(cnt),
                         ctypes.byref(n_out), ctypes.byref(heavy), ctypes.byref(den))
    assert st == rl_amd.RL_OK and (n_out.value, heavy.value, den.value) == (22, 22, wd)
    assert np.array_equal(top[:22], wk[:22]) and np.array_equal(cnt[:22], wc[:22])
    assert np.all(top[22:] == 7) and np.all(cnt[22:] == 7)
    # the unselected call on the same keys does return the hot key: the selector is what removed it
    assert int(e.top_keys(k, 1, 1)[0][0]) == HOT


def test_top_denied_nothing_and_everything(engines):
    e = engines["three"]
    k, p, l, op, al, r = denied_case()
    n = 2049
    l1 = np.full(n, 1, np.uint16)
    none = e.top_denied_device(n, dev(k[:n]), dev(p[:n]), dev(l1), None, dev(np.ones(n, np.uint8)), dev(r[:n]), 1, 8, 1)
    assert (len(none[0]), none[2], none[3]) == (0, 0, 0)
    tk, tc, heavy, den = e.top_denied_device(n, dev(k[:n]), dev(p[:n]), dev(l1), None, dev(np.zeros(n, np.uint8)),
                                             dev(r[:n]), 1, 4096, 1)
    wk, wc, wh = rc.top_model(k[:n], 4096, 1)
    assert den == n and heavy == wh and np.array_equal(tk.cpu().numpy(), wk) and np.array_equal(tc.cpu().numpy(), wc)
    # limiter and op both absent: limiter 0, every request an acquire
    tk, tc, heavy, den = e.top_denied(k[:n], p[:n], None, None, np.zeros(n, np.uint8), r[:n], 0, 4096, 1)
    assert den == n and heavy == wh and np.array_equal(tk, wk) and np.array_equal(tc, wc)
    assert e.top_denied(k[:n], p[:n], None, None, np.zeros(n, np.uint8), r[:n], 1, 4096, 1)[3] == 0
