"""rl_top_keys / rl_top_keys_device on the GPU against numpy: exact keys, counts, n_out and
n_heavy in every case. The expected answer is np.unique + filter + lexsort, the contract's
own definition. Every case runs through the device form; the small ones through the host form
too."""
import ctypes

import numpy as np
import pytest

import rl_amd

pytestmark = pytest.mark.gpu

U64 = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A


def expected(keys, k, min_count):
    """(top keys, top counts, n_heavy): count descending, then key ascending as unsigned."""
    u, c = np.unique(np.asarray(keys, U64), return_counts=True)
    m = c >= min_count
    u, c = u[m], c[m].astype(np.int64)
    order = np.lexsort((u, -c))
    return u[order][:k], c[order][:k].astype(U64), int(u.size)


@pytest.fixture(scope="module")
def eng():
    e = rl_amd.Engine(device=0, max_batch=1 << 16, capacity=1 << 12)
    yield e
    e.close()


def device_form(e, keys, k, min_count):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(keys, U64).view(np.int64)).cuda()
    tk, tc, n_heavy = e.top_keys_device(t, k, min_count)
    return tk.cpu().numpy(), tc.cpu().numpy(), n_heavy


def check(e, keys, k, min_count, host=True):
    keys = np.ascontiguousarray(keys, U64)
    wk, wc, wh = expected(keys, k, min_count)
    forms = [("device", device_form)] + ([("host", lambda e, *a: e.top_keys(*a))] if host else [])
    for name, form in forms:
        gk, gc, gh = form(e, keys, k, min_count)
        assert gh == wh, (name, gh, wh)
        assert gk.shape == wk.shape, (name, gk.shape, wk.shape)     # n_out
        assert np.array_equal(gk, wk), name
        assert np.array_equal(gc, wc), name
    return wk, wc, wh


def test_empty_and_single(eng):
    check(eng, np.zeros(0, U64), 4, 1)
    check(eng, np.array([12345], U64), 4, 1)
    check(eng, np.array([12345], U64), 4, 2)          # nothing qualifies


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_wave_edges(eng, n):
    five = rl_amd.mix64(np.arange(5, dtype=U64))
    keys = five[np.random.default_rng(n).integers(0, 5, n)]
    keys[:5] = five                                    # all five occur
    for min_count in (1, 2):
        for k in (1, 3, 4096):
            check(eng, keys, k, min_count)


def test_one_key_repeated(eng):
    """200,000 copies: ~98 tiles of one key, kept in LDS across a workgroup's tiles and
    flushed once at its end."""
    key = int(rl_amd.mix64(U64(99)))
    wk, wc, wh = check(eng, np.full(200_000, key, U64), 8, 1)
    assert wh == 1 and int(wc[0]) == 200_000


def test_strided_key_accumulates_across_workgroups(eng):
    n = 1 << 20
    keys = rl_amd.mix64(np.arange(n, dtype=U64) + U64(1 << 40))
    hot = U64(0xABCDEF0123456789)
    keys[::4096] = hot                                 # once in every 4096-element stride
    wk, wc, wh = check(eng, keys, 16, 2, host=False)
    assert wh == 1 and int(wk[0]) == int(hot) and int(wc[0]) == n // 4096


def test_extreme_keys(eng):
    ext = np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1], U64)
    keys = np.tile(ext, 7)[np.random.default_rng(3).permutation(35)]
    wk, wc, wh = check(eng, keys, 3, 1)
    assert wk.tolist() == [0, 1, (1 << 63) - 1] and wh == 5     # ascending unsigned at the tie
    wk, wc, wh = check(eng, keys, 4096, 7)
    assert wk.tolist() == ext.tolist() and wc.tolist() == [7] * 5
    # ~0 ahead on count, 0 behind: both are counted like any key
    more = np.concatenate([keys, np.full(3, (1 << 64) - 1, U64), np.zeros(1, U64)])
    wk, wc, wh = check(eng, more, 2, 1)
    assert wk.tolist() == [(1 << 64) - 1, 0] and wc.tolist() == [10, 8]


def _distinct(n, seed):
    return rl_amd.mix64(np.arange(n, dtype=U64) + U64(seed << 32))   # mix64 is a bijection


def test_full_capacity(eng):
    keys = _distinct(rl_amd.TOP_KEYS_CANDIDATES, 5)
    wk, wc, wh = check(eng, keys, 4096, 1, host=False)
    assert wh == 65536 and np.array_equal(wk, np.sort(keys)[:4096]) and np.all(wc == 1)


def test_one_over_capacity_overflows(eng):
    import torch
    keys = _distinct(rl_amd.TOP_KEYS_CANDIDATES + 1, 6)
    with pytest.raises(rl_amd.RlError) as ei:
        eng.top_keys(keys, 4096, 1)
    assert ei.value.status == rl_amd.RL_E_CAPACITY
    with pytest.raises(rl_amd.RlError) as ei:
        device_form(eng, keys, 4096, 1)
    assert ei.value.status == rl_amd.RL_E_CAPACITY
    # the raw calls: hdr = {0, 0, 1, n} and nothing written; *n_out = 0
    L = rl_amd.lib()
    t = torch.from_numpy(keys.view(np.int64)).cuda()
    top = torch.full((4096,), FILL, dtype=torch.int64, device="cuda")
    cnt = torch.full((4096,), FILL, dtype=torch.int64, device="cuda")
    hdr = torch.full((4,), FILL, dtype=torch.int64, device="cuda")
    assert L.rl_top_keys_device(eng.handle, keys.size, rl_amd._p(t), 4096, 1, rl_amd._p(top),
                                rl_amd._p(cnt), rl_amd._p(hdr), None) == rl_amd.RL_OK
    eng.sync()
    assert hdr.cpu().tolist() == [0, 0, 1, keys.size]
    assert bool((top == FILL).all()) and bool((cnt == FILL).all())
    n_out, heavy = ctypes.c_size_t(9), ctypes.c_uint64(9)
    htop = np.full(4096, FILL, U64)
    hcnt = np.full(4096, FILL, U64)
    assert L.rl_top_keys(eng.handle, keys.size, rl_amd._p(keys), 4096, 1, rl_amd._p(htop),
                         rl_amd._p(hcnt), ctypes.byref(n_out), ctypes.byref(heavy)) == rl_amd.RL_E_CAPACITY
    assert n_out.value == 0 and np.all(htop == FILL) and np.all(hcnt == FILL)


@pytest.fixture(scope="module")
def zipf_keys():
    """2^20 keys, Zipf(1.1) ranks rejected above 2^24: 209,602 distinct keys (above the
    candidate cap, so the sketch has to filter), 3,543 with count >= 16, top count 120,401."""
    n = 1 << 20
    rng = np.random.default_rng(7)
    parts, have = [], 0
    while have < n:
        r = rng.zipf(1.1, n)
        r = r[r <= (1 << 24)]
        parts.append(r)
        have += r.size
    return rl_amd.mix64(np.concatenate(parts)[:n].astype(U64))


@pytest.mark.parametrize("k", [1024, 4096])
def test_zipf(eng, zipf_keys, k):
    wk, wc, wh = check(eng, zipf_keys, k, 16, host=(k == 1024))   # host: 16 chunks of max_batch
    assert wh == 3543 and int(wc[0]) == 120_401 and wk.size == min(k, 3543)


def test_entries_beyond_n_out_keep_their_fill(eng):
    import torch
    keys = np.repeat(rl_amd.mix64(np.arange(10, dtype=U64)), np.arange(1, 11))   # counts 1..10
    wk, wc, wh = expected(keys, 16, 4)                                            # 7 qualify
    assert wk.size == 7
    L = rl_amd.lib()
    t = torch.from_numpy(keys.view(np.int64)).cuda()
    top = torch.full((16,), FILL, dtype=torch.int64, device="cuda")
    cnt = torch.full((16,), FILL, dtype=torch.int64, device="cuda")
    hdr = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert L.rl_top_keys_device(eng.handle, keys.size, rl_amd._p(t), 16, 4, rl_amd._p(top),
                                rl_amd._p(cnt), rl_amd._p(hdr), None) == rl_amd.RL_OK
    eng.sync()
    assert hdr.cpu().tolist() == [7, 7, 0, keys.size]
    gt, gc = top.cpu().numpy().view(U64), cnt.cpu().numpy().view(U64)
    assert np.array_equal(gt[:7], wk) and np.array_equal(gc[:7], wc)
    assert np.all(gt[7:] == FILL) and np.all(gc[7:] == FILL)
    # k below n_heavy: the cut is at k, n_heavy still exact
    top.fill_(FILL)
    cnt.fill_(FILL)
    assert L.rl_top_keys_device(eng.handle, keys.size, rl_amd._p(t), 3, 4, rl_amd._p(top),
                                rl_amd._p(cnt), rl_amd._p(hdr), None) == rl_amd.RL_OK
    eng.sync()
    assert hdr.cpu().tolist() == [3, 7, 0, keys.size]
    gt, gc = top.cpu().numpy().view(U64), cnt.cpu().numpy().view(U64)
    assert np.array_equal(gt[:3], wk[:3]) and np.all(gt[3:] == FILL) and np.all(gc[3:] == FILL)
    # the host form
    htop, hcnt = np.full(16, FILL, U64), np.full(16, FILL, U64)
    n_out, heavy = ctypes.c_size_t(0), ctypes.c_uint64(0)
    assert L.rl_top_keys(eng.handle, keys.size, rl_amd._p(keys), 16, 4, rl_amd._p(htop), rl_amd._p(hcnt),
                         ctypes.byref(n_out), ctypes.byref(heavy)) == rl_amd.RL_OK
    assert (n_out.value, heavy.value) == (7, 7)
    assert np.array_equal(htop[:7], wk) and np.all(htop[7:] == FILL) and np.all(hcnt[7:] == FILL)


def test_each_invalid_argument_alone(eng):
    """With a live engine every other argument is fine, so each check is seen on its own."""
    L = rl_amd.lib()
    keys = np.array([1, 2, 2], U64)
    top, cnt, hdr = (np.full(4, FILL, U64) for _ in range(3))
    n_out, heavy = ctypes.c_size_t(9), ctypes.c_uint64(9)
    p = rl_amd._p
    bad = rl_amd.RL_E_INVALID_ARG
    h = eng.handle
    for k, mc, kp in ((0, 1, p(keys)), (4097, 1, p(keys)), (4, 0, p(keys)), (4, 1, None)):
        assert L.rl_top_keys(h, 3, kp, k, mc, p(top), p(cnt), ctypes.byref(n_out), ctypes.byref(heavy)) == bad
        assert L.rl_top_keys_device(h, 3, kp, k, mc, p(top), p(cnt), p(hdr), None) == bad
    assert L.rl_top_keys(h, 3, p(keys), 4, 1, None, p(cnt), ctypes.byref(n_out), ctypes.byref(heavy)) == bad
    assert L.rl_top_keys(h, 3, p(keys), 4, 1, p(top), p(cnt), None, ctypes.byref(heavy)) == bad
    assert L.rl_top_keys_device(h, 3, p(keys), 4, 1, p(top), p(cnt), None, None) == bad
    assert L.rl_top_keys(h, (1 << 31) + 1, p(keys), 4, 1, p(top), p(cnt), ctypes.byref(n_out),
                         ctypes.byref(heavy)) == bad
    assert all(np.all(a == FILL) for a in (top, cnt, hdr)) and n_out.value == 9 and heavy.value == 9


def test_queries_leave_batches_statistics_and_status_alone():
    """The same two batches on two engines, one of them with queries in between (and one
    before its first batch): same decisions, same rl_batch_stats, same rl_last_status."""
    rng = np.random.default_rng(11)
    n = 4096
    ks = rl_amd.mix64(rng.integers(0, 300, 2 * n).astype(U64))
    permits = rng.integers(0, 4, 2 * n).astype(np.int32)            # some invalid (0)
    now = (1_700_000_000_000 + np.arange(2 * n, dtype=np.int64) // 8) * 1_000_000
    out = []
    for query in (False, True):
        e = rl_amd.Engine(device=0, max_batch=n, capacity=1 << 12)
        e.add_limiter(rl_amd.TB, 50, 60000, 10.0)
        if query:
            e.top_keys(ks, 8, 2)                                    # 2 chunks of max_batch
        r1 = e.execute(ks[:n], permits[:n], now[:n])
        s1, st1 = e.stats(), e.last_status()
        if query:
            gk, gc, gh = e.top_keys(ks, 16, 2)
            wk, wc, wh = expected(ks, 16, 2)
            assert np.array_equal(gk, wk) and np.array_equal(gc, wc) and gh == wh
            device_form(e, ks, 16, 2)
            assert e.stats() == s1 and e.last_status() == st1
        r2 = e.execute(ks[n:], permits[n:], now[n:])
        out.append((r1, s1, st1, r2, e.stats(), e.last_status()))
        e.close()
    (a1, as1, ast1, a2, as2, ast2), (b1, bs1, bst1, b2, bs2, bst2) = out
    assert ast1 == bst1 == rl_amd.RL_E_INVALID_REQUEST and ast2 == bst2
    assert as1 == bs1 and as2 == bs2
    for x, y in ((a1, b1), (a2, b2)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[3] == y[3]
        assert np.array_equal(x[2].view(U64), y[2].view(U64))
