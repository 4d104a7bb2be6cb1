"""Whole-table snapshot and restore (rl_snapshot_keys(_device), rl_put_keys_device,
rl_restore_keys): a limiter's table leaves as images in (region, slot) order, chunk by chunk, and
an engine restored from them decides exactly as the original, the local-cache word included.

The engines have the three limiters of test_gpu_migrate.py: a token bucket with fractional
refill, a sliding window, and a sliding window with the local cache on. A limiter's smallest table
has MIN_REGIONS = 8 regions; about 110 keys fall into each of regions 0 and 1 and a handful into
region 7, so probe chains collide, most other regions are empty, and nothing grows. The state at
the snapshot holds key_hash 0 and ~0 under all three limiters, a key blocked only by the cache
word, a token bucket that was reset (a tombstone: no image) and a sliding-window key with both
buckets.
"""
import numpy as np
import pytest
import torch

import rl_amd
from oracle.rl_oracle import PyOracle

pytestmark = pytest.mark.gpu

NS = 1_000_000
T0 = 1_700_000_000_000                     # a multiple of both windows
W = 4000
LIMS = [dict(algo=rl_amd.TB, max_permits=10, window_ms=W, refill_per_s=2.5),
        dict(algo=rl_amd.SW, max_permits=6, window_ms=W),
        dict(algo=rl_amd.SW, max_permits=3, window_ms=W, local_cache_ttl_ms=3000)]
K_BLOCK, K_RESET, K_NOSTATE, K_BOTH = 0xB10C, 0x7E5E7, 0xAB5E27, 0xB074
ALL1 = np.uint64(0xFFFFFFFFFFFFFFFF)
BITS = rl_amd.MIN_REGIONS.bit_length() - 1
IMG = rl_amd.KEY_IMAGE_DTYPE
SENT = 0xA5


def make(**kw):
    kw.setdefault("max_batch", 1 << 16)
    e = rl_amd.Engine(capacity=1, **kw)
    for l in LIMS:
        e.add_limiter(capacity=1, **l)
    return e


def oracle():
    o = PyOracle()
    for l in LIMS:
        o.add_limiter(**l)
    return o


def region_of(key_hash, bits=BITS):
    return (rl_amd.mix64(key_hash) >> np.uint64(64 - bits)).astype(np.int64)


def region_keys(lim):
    """Distinct keys (per limiter): 110 in each of regions 0 and 1 of the smallest table, 5 in region 7."""
    cand = np.arange(1, 200_000, dtype=np.uint64) + np.uint64(lim * 1_000_000)
    reg = region_of(cand)
    return np.concatenate([cand[reg == 0][:110], cand[reg == 1][:110], cand[reg == 7][:5]])


def traffic(seed, keysets, n, t_lo, t_hi, special=()):
    """n random acquires over the limiters' key sets (+ key 0 and ~0 under every limiter) and
    the hand-made `special` requests (key, permits, now_ms, limiter, op), in time order."""
    rng = np.random.default_rng(seed)
    lim = rng.integers(0, len(LIMS), n)
    keys = np.array([keysets[l][rng.integers(0, keysets[l].size)] for l in lim], np.uint64)
    shared = rng.random(n)
    keys[shared < 0.02] = 0
    keys[(shared >= 0.02) & (shared < 0.04)] = ALL1
    now = rng.integers(t_lo, t_hi, n)
    permits = rng.integers(1, 3, n)
    ops = np.zeros(n, np.int64)
    if special:
        sp = np.array(special, dtype=object)
        keys = np.concatenate([keys, sp[:, 0].astype(np.uint64)])
        permits = np.concatenate([permits, sp[:, 1].astype(np.int64)])
        now = np.concatenate([now, sp[:, 2].astype(np.int64)])
        lim = np.concatenate([lim, sp[:, 3].astype(np.int64)])
        ops = np.concatenate([ops, sp[:, 4].astype(np.int64)])
    order = np.argsort(now, kind="stable")
    return (keys[order], permits[order].astype(np.int32), (now[order] * NS).astype(np.int64),
            lim[order].astype(np.uint16), ops[order].astype(np.uint8))


SPECIAL1 = (
    # three allows late in window [T0, T0 + W): the third one's count (3 >= max) goes into the
    # local cache, which blocks the key until T0 + 3902 + 3000
    [(K_BLOCK, 1, T0 + 3900 + i, 2, 0) for i in range(3)] +
    [(K_BOTH, 1, T0 + 3000, 1, 0), (K_BOTH, 1, T0 + 4500, 1, 0)] +
    [(K_RESET, 2, T0 + 3000, 0, 0), (K_RESET, 1, T0 + 3500, 0, rl_amd.OP_RESET)])
# at T0 + 6000 the estimate of K_BLOCK is (long)(3 * 0.5) = 1: only the cache word denies it
SPECIAL2 = [(K_BLOCK, 1, T0 + 6000, 2, 0), (K_BOTH, 1, T0 + 6100, 1, 0), (K_RESET, 3, T0 + 6200, 0, 0),
            (K_NOSTATE, 1, T0 + 6300, 0, 0), (K_NOSTATE, 1, T0 + 6300, 2, 0)]
KEYSETS = [region_keys(l) for l in range(len(LIMS))]
EVERY = np.unique(np.concatenate(KEYSETS + [np.array([0, ALL1, K_BOTH, K_BLOCK, K_RESET, K_NOSTATE],
                                                     np.uint64)]))
TR1 = traffic(12, KEYSETS, 3000, T0 + 2500, T0 + 5500, SPECIAL1)
TR2 = traffic(22, KEYSETS, 3000, T0 + 5600, T0 + 7000, SPECIAL2)


def run(e, tr):
    a, r, t, st = e.execute(*tr)
    assert st == rl_amd.RL_OK, rl_amd.strerror(st)
    return a, r, t


def assert_same(got, want, what):
    np.testing.assert_array_equal(got[0], np.asarray(want[0], np.uint8), err_msg=what)
    np.testing.assert_array_equal(got[1], np.asarray(want[1], np.int64), err_msg=what)
    gt, wt = np.asarray(got[2], np.float64), np.asarray(want[2], np.float64)
    m = ~np.isnan(wt)
    np.testing.assert_array_equal(gt[m].view(np.uint64), wt[m].view(np.uint64), err_msg=what)


def source():
    """Engine A after batch 1 (nothing grew)."""
    A = make()
    run(A, TR1)
    assert [A.limiter_slots(l) for l in range(len(LIMS))] == [rl_amd.MIN_REGIONS * rl_amd.REGION_SLOTS] * 3
    return A


def by_key(imgs):
    return imgs[np.lexsort((imgs["key_hash"], imgs["limiter"]))]


def whole(e, lim, chunk=1 << 12):
    parts = list(e.snapshot(lim, chunk=chunk))
    return np.concatenate(parts) if parts else np.zeros(0, IMG)


def whole_all(e, chunk=1 << 12):
    return np.concatenate([whole(e, l, chunk) for l in range(len(LIMS))])


def sentinel_buf(cap):
    out = np.zeros(cap, IMG)
    out.view(np.uint8)[:] = SENT
    return out


def untouched(buf):
    return bool(np.all(buf.view(np.uint8) == SENT))


def to_device(imgs):
    a = np.ascontiguousarray(imgs, IMG)
    words = a.view(np.int64) if a.shape[0] else np.zeros(6, np.int64)
    return torch.from_numpy(words.copy()).cuda()


def put_device(e, imgs):
    """rl_put_keys_device of host images uploaded with torch; returns the header as a list."""
    hdr = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    dev = to_device(imgs)
    torch.cuda.synchronize()                                # the fills above run on torch's stream
    e.put_keys_device(imgs.shape[0], dev, hdr)
    e.sync()
    return [int(x) for x in hdr.cpu()]


def snap_device(e, lim, begin, count, cap):
    """rl_snapshot_keys_device into a sentinel-filled device buffer; (images[cap], header)."""
    out = torch.from_numpy(sentinel_buf(max(cap, 1)).view(np.int64).copy()).cuda()
    hdr = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                                # the fills above run on torch's stream
    e.snapshot_keys_device(lim, begin, count, out, cap, hdr)
    e.sync()
    return out.cpu().numpy().view(IMG)[:cap], [int(x) for x in hdr.cpu()]


def as_tuples(ex):
    return [(int(x["limiter"]), int(x["key_hash"]), int(x["kind"]), int(x["window_start_ms"]),
             int(x["count"]), float(x["tokens"]).hex(), int(x["last_refill_ms"]),
             int(x["expire_at_ms"])) for x in ex]


def test_snapshot_equals_copy_keys_in_region_order():
    A = source()
    ref = A.copy_keys(EVERY)                                # sorted by (limiter, key_hash)
    assert ref.shape[0] > 500
    for lim in range(len(LIMS)):
        got = np.concatenate(list(A.snapshot(lim, chunk=256)))
        assert np.all(got["limiter"] == lim) and not got["reserved"].any()
        assert by_key(got).tobytes() == ref[ref["limiter"] == lim].tobytes()
        reg = region_of(got["key_hash"])
        assert np.all(np.diff(reg) >= 0)
        assert {0, 1, 7} <= set(reg.tolist())
        keys = set(got["key_hash"].tolist())
        assert {0, int(ALL1)} <= keys
        assert K_NOSTATE not in keys and K_RESET not in keys            # never seen; a tombstone
    blk = whole(A, 2)
    blk = blk[blk["key_hash"] == K_BLOCK]
    assert blk.shape[0] == 1 and int(blk["cache_word"][0]) == T0 + 3902 + 3000
    both = whole(A, 1)
    both = both[both["key_hash"] == K_BOTH]["word"][:, 1]
    assert both.shape[0] == 1 and (int(both[0]) & 0xFFFFFFFF) and (int(both[0]) >> 32)
    with pytest.raises(rl_amd.RlError) as ei:
        A.snapshot_keys(len(LIMS), 0, 1, 256)               # an unknown limiter
    assert ei.value.status == rl_amd.RL_E_INVALID_ARG
    A.close()


@pytest.mark.parametrize("lim", range(len(LIMS)))
def test_chunking_does_not_change_the_array(lim):
    A = source()
    big, st, n, done, total = A.snapshot_keys(lim, 0, 1 << 40, 4096)
    assert (st, done, total) == (rl_amd.RL_OK, 8, 8) and n > 220
    want = big[:n].tobytes()

    def chunked(call, count, cap):
        parts, at = [], 0
        while at < 8:
            imgs, k, d = call(at, count, cap)
            assert 1 <= d <= count
            parts.append(imgs[:k])
            at += d
        assert at == 8
        return np.concatenate(parts).tobytes()

    def host(at, count, cap):
        imgs, st, k, d, tot = A.snapshot_keys(lim, at, count, cap)
        assert st == rl_amd.RL_OK and tot == 8
        return imgs, k, d

    def device(at, count, cap):
        imgs, hdr = snap_device(A, lim, at, count, cap)
        assert hdr[2] == 8 and hdr[3] == 0
        assert untouched(imgs[hdr[0]:])
        return imgs, hdr[0], hdr[1]

    for call in (host, device):
        assert chunked(call, 1, 256) == want                # one region per call
        assert chunked(call, 3, 4096) == want
        assert chunked(call, 8, 128) == want                # the cap cuts regions 0 and 1 apart
    imgs, hdr = snap_device(A, lim, 0, 1 << 40, 4096)
    assert hdr == [n, 8, 8, 0] and imgs[:n].tobytes() == want
    A.close()


def test_the_cut_writes_whole_regions_only():
    A = source()
    for lim in range(len(LIMS)):
        full = whole(A, lim)
        reg = region_of(full["key_hash"])
        c0, c1 = int(np.sum(reg == 0)), int(np.sum(reg == 1))
        assert c0 >= 110 and c1 >= 110
        for cap in (c0, c0 + c1 - 1):
            out = sentinel_buf(cap)
            _, st, n, done, total = A.snapshot_keys(lim, 0, 8, cap, out=out)
            assert (st, n, done, total) == (rl_amd.RL_OK, c0, 1, 8)
            assert out[:n].tobytes() == full[:c0].tobytes() and untouched(out[n:])
            imgs, hdr = snap_device(A, lim, 0, 8, cap)
            assert hdr == [c0, 1, 8, 0]
            assert imgs[:c0].tobytes() == full[:c0].tobytes() and untouched(imgs[c0:])
        for cap in (c0 - 1, 0):
            out = sentinel_buf(max(cap, 1))
            _, st, n, done, total = A.snapshot_keys(lim, 0, 8, cap, out=out)
            assert (st, n, done, total) == (rl_amd.RL_E_TOO_LARGE, c0, 0, 8) and untouched(out)
            imgs, hdr = snap_device(A, lim, 0, 8, cap)
            assert hdr == [0, 0, 8, c0] and untouched(imgs)
        for begin in (8, 9, 1 << 50):
            out = sentinel_buf(256)
            _, st, n, done, total = A.snapshot_keys(lim, begin, 8, 256, out=out)
            assert (st, n, done, total) == (rl_amd.RL_OK, 0, 0, 8) and untouched(out)
            imgs, hdr = snap_device(A, lim, begin, 8, 256)
            assert hdr == [0, 0, 8, 0] and untouched(imgs)
        _, st, n, done, total = A.snapshot_keys(lim, 6, 1 << 60, 256)     # clipped to the table
        assert (st, done, total) == (rl_amd.RL_OK, 2, 8)
        assert A.snapshot_keys(lim, 3, 0, 256)[1:] == (rl_amd.RL_OK, 0, 0, 8)   # an empty range
    A.close()


def test_snapshot_only_reads():
    A = make()
    tr = list(TR1)
    tr[1] = tr[1].copy()
    tr[1][5] = 0                                            # one invalid request
    a, r, t, st = A.execute(*tr)
    assert st == rl_amd.RL_E_INVALID_REQUEST
    stats = A.stats()
    ex = [as_tuples(A.export_state(t * NS)) for t in (T0 + 5500, T0 + 7000)]
    imgs = A.copy_keys(EVERY)
    for lim in range(len(LIMS)):
        whole(A, lim, chunk=256)
        snap_device(A, lim, 0, 8, 4096)
        snap_device(A, lim, 0, 8, 3)
    assert A.stats() == stats
    assert [as_tuples(A.export_state(t * NS)) for t in (T0 + 5500, T0 + 7000)] == ex
    assert A.copy_keys(EVERY).tobytes() == imgs.tobytes()
    assert A.last_status() == rl_amd.RL_E_INVALID_REQUEST
    A.close()


def test_a_clone_decides_as_the_original():
    A, o = make(), oracle()
    assert_same(run(A, TR1), o.run(*TR1), "batch 1 vs oracle")
    imgs8 = whole_all(A, chunk=256)
    for l in range(len(LIMS)):
        A.grow_limiter(l, 4096)                             # 4x: 32 regions
    assert all(A.snapshot_keys(l, 0, 0, 0)[4] == 32 for l in range(len(LIMS)))
    imgs32 = whole_all(A, chunk=256)
    assert by_key(imgs32).tobytes() == by_key(imgs8).tobytes()
    assert imgs32.tobytes() != imgs8.tobytes()
    n = imgs8.shape[0]

    B1, B2, B3, B4 = make(), make(), make(), make(max_batch=256)
    assert put_device(B1, imgs8) == [n, 0, 0, n]            # the same geometry
    assert put_device(B2, imgs32) == [n, 0, 0, n]           # fewer regions than the source: ordered
    for l in range(len(LIMS)):
        B3.grow_limiter(l, 2048)                            # 2x beyond the source of imgs8
    assert put_device(B3, imgs8) == [0, 0, rl_amd.PUT_REJECT_ORDER, n]
    assert B3.copy_keys(EVERY).shape[0] == 0 and B3.export_state(T0 * NS).shape[0] == 0
    assert B3.restore_keys(imgs8) == (rl_amd.RL_OK, n)      # the path of rl_put_keys
    assert B4.restore_keys(imgs32) == (rl_amd.RL_OK, n)     # ordered, in pieces of 256 images
    clones = {"B1": B1, "B2": B2, "B3": B3}

    ref = A.copy_keys(EVERY)
    ex = as_tuples(A.export_state((T0 + 5500) * NS))
    assert ref.shape[0] == n and len(ex) > 0
    for name, B in dict(clones, B4=B4).items():
        assert B.copy_keys(EVERY).tobytes() == ref.tobytes(), name
        assert as_tuples(B.export_state((T0 + 5500) * NS)) == ex, name
        assert B.stats()["n"] == 0 and B.last_status() == rl_amd.RL_OK
    assert [B3.limiter_slots(l) for l in range(3)] == [16 * rl_amd.REGION_SLOTS] * 3   # a put never grows

    want = run(A, TR2)
    assert_same(want, o.run(*TR2), "batch 2, A vs oracle")
    i = np.nonzero((TR2[0] == K_BLOCK) & (TR2[3] == 2))[0]
    assert i.size == 1 and want[0][i[0]] == 0               # denied by the cache word alone
    ref = A.copy_keys(EVERY)
    ex = as_tuples(A.export_state((T0 + 7000) * NS))
    for name, B in clones.items():
        assert_same(run(B, TR2), want, "batch 2, " + name)
        assert B.copy_keys(EVERY).tobytes() == ref.tobytes(), name
        assert as_tuples(B.export_state((T0 + 7000) * NS)) == ex, name
    for e in (A, B1, B2, B3, B4):
        e.close()


def test_a_put_replaces_and_leaves_other_keys_alone():
    A, B = source(), make()
    K_ONLY_B = np.uint64(0x0B0B0B)
    have = A.copy_keys(KEYSETS[1])["key_hash"]              # keys of limiter 1 that A holds state for
    reg = region_of(have)
    mine = np.concatenate([have[reg == 0][:10], have[reg == 1][:10], [K_ONLY_B]]).astype(np.uint64)
    m = mine.size
    run(B, (mine, np.full(m, 2, np.int32), np.full(m, (T0 + 2600) * NS, np.int64),
            np.full(m, 1, np.uint16), np.zeros(m, np.uint8)))
    before = B.copy_keys(mine)
    assert before.shape[0] == m
    a_has = A.copy_keys(mine[:-1])
    assert a_has.shape[0] == 20 and A.copy_keys(mine[-1:]).shape[0] == 0
    assert before[before["key_hash"] != K_ONLY_B].tobytes() != a_has.tobytes()
    imgs = whole_all(A)
    assert put_device(B, imgs) == [imgs.shape[0], 0, 0, imgs.shape[0]]
    assert B.copy_keys(mine[:-1]).tobytes() == a_has.tobytes()
    assert B.copy_keys(mine[-1:]).tobytes() == before[before["key_hash"] == K_ONLY_B].tobytes()
    assert B.copy_keys(EVERY).tobytes() == A.copy_keys(EVERY).tobytes()
    assert whole_all(B).shape[0] == imgs.shape[0] + 1
    A.close()
    B.close()


def synthetic(keys, lim=0):
    """Token-bucket images (5 tokens, refilled at T0) for the given key hashes."""
    imgs = np.zeros(keys.size, IMG)
    imgs["key_hash"] = keys
    imgs["word"][:, 0] = np.float64(5.0).view(np.uint64)
    imgs["word"][:, 1] = T0
    imgs["word"][:, 2] = 1
    imgs["limiter"] = lim
    return imgs


def test_a_full_region_reports_capacity():
    cand = np.arange(1, 400_000, dtype=np.uint64)
    r0 = cand[region_of(cand) == 0][:rl_amd.REGION_SLOTS + 1]
    imgs = synthetic(r0)
    n = imgs.shape[0]
    F, G = make(fixed_capacity=True), make(fixed_capacity=True)
    assert put_device(F, imgs) == [n - 1, 1, 0, n]
    assert G.restore_keys(imgs) == (rl_amd.RL_E_CAPACITY, n - 1)
    for e in (F, G):
        assert e.copy_keys(r0).tobytes() == by_key(imgs[:-1]).tobytes()      # the 257th found no slot
        assert put_device(e, imgs[:3]) == [3, 0, 0, 3]                       # replacing needs no free slot
        out, st, k, done, total = e.snapshot_keys(0, 0, 1, 256)
        assert (st, k, done, total) == (rl_amd.RL_OK, 256, 1, 8)             # an exact fit
        assert by_key(out).tobytes() == by_key(imgs[:-1]).tobytes()
        out = sentinel_buf(255)
        assert e.snapshot_keys(0, 0, 1, 255, out=out)[1:] == (rl_amd.RL_E_TOO_LARGE, 256, 0, 8)
        assert untouched(out)
        assert snap_device(e, 0, 0, 8, 255)[1] == [0, 0, 8, 256]
        assert snap_device(e, 0, 0, 8, 256)[1] == [256, 8, 8, 0]
        assert e.limiter_slots(0) == rl_amd.MIN_REGIONS * rl_amd.REGION_SLOTS
        e.close()


def test_duplicates_and_unknown_limiters():
    B = make()
    cand = np.arange(1, 100_000, dtype=np.uint64)
    k0 = cand[region_of(cand) == 0][:3]
    imgs = synthetic(np.array([k0[0], k0[1], k0[0], k0[2], k0[0]], np.uint64))
    imgs["word"][:, 1] = T0 + np.arange(5)                   # the copies of k0[0] differ
    assert put_device(B, imgs) == [5, 0, 0, 5]
    got = B.copy_keys(k0)
    assert got.tobytes() == by_key(imgs[[4, 1, 3]]).tobytes()     # the last one in array order wins
    assert B.restore_keys(imgs[[0, 1, 3]]) == (rl_amd.RL_OK, 3)
    assert B.copy_keys(k0).tobytes() == by_key(imgs[[0, 1, 3]]).tobytes()

    C = make()
    bad = synthetic(k0)
    bad["limiter"][2] = len(LIMS)
    hdr = put_device(C, bad)
    assert hdr[0] == 0 and hdr[1] == 0 and hdr[2] & rl_amd.PUT_REJECT_LIMITER and hdr[3] == 3
    assert C.copy_keys(k0).shape[0] == 0
    bad["limiter"][:] = [2, 0, len(LIMS)]                    # out of order as well
    hdr = put_device(C, bad)
    assert hdr[0] == 0 and hdr[2] == rl_amd.PUT_REJECT_LIMITER | rl_amd.PUT_REJECT_ORDER
    assert C.copy_keys(k0).shape[0] == 0
    with pytest.raises(rl_amd.RlError) as ei:
        C.restore_keys(bad)
    assert ei.value.status == rl_amd.RL_E_INVALID_ARG and C.copy_keys(k0).shape[0] == 0
    assert put_device(C, bad[:0]) == [0, 0, 0, 0]
    assert C.restore_keys(bad[:0]) == (rl_amd.RL_OK, 0)
    B.close()
    C.close()


def test_the_snapshot_follows_a_growth():
    A = source()
    before = whole_all(A)
    for l in range(len(LIMS)):
        assert A.snapshot_keys(l, 0, 0, 0)[4] == 8
        A.grow_limiter(l, 2048)
        assert A.snapshot_keys(l, 0, 0, 0)[4] == 16 == A.limiter_slots(l) // rl_amd.REGION_SLOTS
    after = whole_all(A, chunk=256)
    assert by_key(after).tobytes() == by_key(before).tobytes()
    for l in range(len(LIMS)):
        part = after[after["limiter"] == l]
        assert np.all(np.diff(region_of(part["key_hash"], BITS + 1)) >= 0)
    A.close()
