"""Key migration between engines (rl_copy_keys / rl_drop_keys / rl_put_keys): the state of a
listed set of keys moves bit for bit, the local-cache word included, so the engines that share
a keyspace after the move decide exactly as one engine on the whole stream.

Engines A, B and C have the same three limiters: a token bucket with fractional refill, a
sliding window, and a sliding window with the local cache on. One batch builds state on A; half
of the keys then move to B; C runs every batch itself and is the reference, beside the Python
oracle. A limiter's smallest table has MIN_REGIONS regions, so "a table of one (two) regions" is
made by choosing keys whose tags all fall into region 0 (regions 0 and 1) of that table: about
110 keys per 256-slot region share its 64 home buckets, so probe chains collide, and the table
does not grow (a region grows beyond 160 used slots).

The state at the move holds: sliding-window keys with both buckets, a key blocked by the local
cache whose window estimate alone would let it through in the next batch, a token bucket that
was reset (a tombstone: no image), a listed key that was never seen, key_hash 0 under all three
limiters and key_hash ~0.
"""
import numpy as np
import pytest

import rl_amd
from oracle.rl_oracle import PyOracle

pytestmark = pytest.mark.gpu

NS = 1_000_000
T0 = 1_700_000_000_000                     # a multiple of both windows
W = 4000
LIMS = [dict(algo=rl_amd.TB, max_permits=10, window_ms=W, refill_per_s=2.5),
        dict(algo=rl_amd.SW, max_permits=6, window_ms=W),
        dict(algo=rl_amd.SW, max_permits=3, window_ms=W, local_cache_ttl_ms=3000)]
T_MOVE = T0 + 5500                         # nothing written in batch 1 has expired by then
K_BLOCK, K_RESET, K_NOSTATE, K_BOTH = 0xB10C, 0x7E5E7, 0xAB5E27, 0xB074
ALL1 = np.uint64(0xFFFFFFFFFFFFFFFF)
BITS = rl_amd.MIN_REGIONS.bit_length() - 1


def make(**kw):
    e = rl_amd.Engine(max_batch=1 << 16, capacity=1, **kw)
    for l in LIMS:
        e.add_limiter(capacity=1, **l)
    return e


def oracle():
    o = PyOracle()
    for l in LIMS:
        o.add_limiter(**l)
    return o


def region_keys(lim, regions, per_region):
    """Distinct keys (per limiter) whose tags fall into regions [0, regions) of the smallest table."""
    cand = np.arange(1, 200_000, dtype=np.uint64) + np.uint64(lim * 1_000_000)
    reg = rl_amd.mix64(cand) >> np.uint64(64 - BITS)
    return np.concatenate([cand[reg == r][:per_region] for r in range(regions)])


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


def as_tuples(ex):
    return [(int(x["limiter"]), int(x["key_hash"]), int(x["kind"]), int(x["window_start_ms"]),
             int(x["count"]), float(x["tokens"]).hex(), int(x["last_refill_ms"]),
             int(x["expire_at_ms"])) for x in ex]


def merged_export(now_ms, *engines):
    out = []
    for e in engines:
        out += as_tuples(e.export_state(now_ms * NS))
    out.sort(key=lambda x: (x[0], x[1], x[3]))
    return out


def usage_sum(now_ms, *engines):
    tot = {}
    for li in range(len(LIMS)):
        for f in ("live_keys", "redis_keys", "cache_blocked", "used_permits"):
            tot[li, f] = sum(e.limiter_usage(li, now_ms * NS)[f] for e in engines)
    return tot


def split_run(tr, moved, on_moved, on_rest):
    """The batch with the moved keys' requests on one engine and the rest on the other, merged
    back into arrival order."""
    m = np.isin(tr[0], moved)
    a = np.zeros(tr[0].size, np.uint8)
    r = np.zeros(tr[0].size, np.int64)
    t = np.zeros(tr[0].size, np.float64)
    for mask, e in ((m, on_moved), (~m, on_rest)):
        a[mask], r[mask], t[mask] = run(e, tuple(x[mask] for x in tr))
    return (a, r, t), m


@pytest.mark.parametrize("regions", [1, 2])
def test_moved_keys_decide_as_one_engine(regions):
    A, B, C, o = make(), make(), make(), oracle()
    keysets = [region_keys(l, regions, 110) for l in range(len(LIMS))]
    tr1 = traffic(11 + regions, keysets, 3000, T0 + 2500, T0 + 5500, SPECIAL1)
    got = run(A, tr1)
    assert_same(got, run(C, tr1), "batch 1, A vs C")
    assert_same(got, o.run(*tr1), "batch 1 vs oracle")
    slots = [A.limiter_slots(l) for l in range(len(LIMS))]
    assert slots == [rl_amd.MIN_REGIONS * rl_amd.REGION_SLOTS] * len(LIMS)      # nothing grew

    every = np.unique(np.concatenate(keysets + [np.array([0, ALL1, K_BOTH], np.uint64)]))
    moved = np.unique(np.concatenate([every[::2], np.array([0, K_BLOCK, K_RESET, K_NOSTATE], np.uint64)]))
    stay = np.setdiff1d(every, moved)
    assert moved.size > 150 * regions and stay.size > 150 * regions

    # ---- (a) the images: what the oracle's keyspace holds for the moved keys, sorted
    before = (A.stats(), B.stats())
    imgs = A.copy_keys(np.concatenate([moved, moved[:7]]))            # duplicates count once
    ks = o.keyspace(T_MOVE)
    mset = set(moved.tolist())
    want = sorted({(k[0], k[1]) for k in ks if int(k[1]) in mset})
    assert [(int(x["limiter"]), int(x["key_hash"])) for x in imgs] == want
    have = set(want)
    assert {(0, 0), (1, 0), (2, 0)} <= have                          # one hash under all three limiters
    assert (2, K_BLOCK) in have and (0, K_RESET) not in have
    assert not any(k == K_NOSTATE for _, k in have)
    both = imgs[imgs["limiter"] == 1]["word"][:, 1]
    assert np.any(((both & np.uint64(0xFFFFFFFF)) != 0) & ((both >> np.uint64(32)) != 0))
    blk = imgs[(imgs["limiter"] == 2) & (imgs["key_hash"] == K_BLOCK)]
    assert blk.shape[0] == 1 and int(blk["cache_word"][0]) == T0 + 3902 + 3000
    assert np.all(imgs[imgs["limiter"] != 2]["cache_word"] == 0)

    # ---- (h) a buffer that is too small: the exact count, nothing written
    out, st, n_out = A.copy_keys(moved, cap=imgs.shape[0] - 1)
    assert st == rl_amd.RL_E_TOO_LARGE and n_out == imgs.shape[0]
    assert not out.view(np.uint8).any()
    out, st, n_out = A.copy_keys(moved, cap=0)
    assert st == rl_amd.RL_E_TOO_LARGE and n_out == imgs.shape[0]

    # ---- the move
    assert B.put_keys(imgs) == (rl_amd.RL_OK, imgs.shape[0])
    assert A.drop_keys(moved) == imgs.shape[0]
    assert (A.stats(), B.stats()) == before                           # (j) no batch statistic moved

    # ---- (f) the dropped keys are gone from A, present on B, bit for bit
    assert A.copy_keys(moved).shape[0] == 0
    assert A.drop_keys(moved) == 0
    assert B.copy_keys(moved).tobytes() == imgs.tobytes()
    assert B.copy_keys(stay).shape[0] == 0

    # ---- (b), (c) the two keyspaces together are C's
    for now in (T_MOVE, T_MOVE + 2000):
        assert merged_export(now, A, B) == merged_export(now, C)
        assert merged_export(now, C) == [k[:5] + (float(k[5]).hex(),) + k[6:] for k in o.keyspace(now)]
        assert usage_sum(now, A, B) == usage_sum(now, C)
    assert usage_sum(T_MOVE, B)[2, "cache_blocked"] >= 1

    # ---- (d), (e) the next batch: moved keys on B, the rest on A
    tr2 = traffic(21 + regions, keysets, 3000, T0 + 5600, T0 + 7000, SPECIAL2)
    want2 = run(C, tr2)
    assert_same(want2, o.run(*tr2), "batch 2, C vs oracle")
    got2, m = split_run(tr2, moved, B, A)
    assert_same(got2, want2, "batch 2, A + B vs C")
    assert_same(tuple(x[~m] for x in got2), tuple(x[~m] for x in want2), "keys that stayed on A")
    i = np.nonzero((tr2[0] == K_BLOCK) & (tr2[3] == 2))[0]
    assert i.size == 1 and got2[0][i[0]] == 0                         # denied by the cache word alone
    assert merged_export(T0 + 7000, A, B) == merged_export(T0 + 7000, C)

    # ---- (g) moving them back restores the single keyspace
    back = B.copy_keys(moved)
    assert A.put_keys(back) == (rl_amd.RL_OK, back.shape[0])
    assert B.drop_keys(moved) == back.shape[0]
    assert merged_export(T0 + 7000, A) == merged_export(T0 + 7000, C)
    assert merged_export(T0 + 7000, B) == []
    assert usage_sum(T0 + 7000, A) == usage_sum(T0 + 7000, C)
    tr3 = traffic(31 + regions, keysets, 2000, T0 + 7000, T0 + 9000)
    assert_same(run(A, tr3), run(C, tr3), "batch 3 after the move back")
    for e in (A, B, C):
        e.close()


def test_put_into_a_full_fixed_region_reports_capacity():
    """(i) RL_E_CAPACITY from a put into a full region of a fixed-capacity table; the images
    bound for other regions are put."""
    G, F = make(), make(fixed_capacity=True)
    G.grow_limiter(0, 4096)                     # the source spreads region 0's keys over four
    cand = np.arange(1, 400_000, dtype=np.uint64)
    reg = rl_amd.mix64(cand) >> np.uint64(64 - BITS)
    r0, r1 = cand[reg == 0][:266], cand[reg == 1][:5]
    keys = np.concatenate([r0, r1])
    n = keys.size
    run(G, (keys, np.ones(n, np.int32), np.full(n, T0 * NS, np.int64), np.zeros(n, np.uint16),
            np.zeros(n, np.uint8)))
    imgs = G.copy_keys(keys)
    assert imgs.shape[0] == n
    in0 = np.isin(imgs["key_hash"], r0)
    fill, rest = imgs[in0][:rl_amd.REGION_SLOTS], np.concatenate([imgs[in0][rl_amd.REGION_SLOTS:], imgs[~in0]])
    assert F.put_keys(fill) == (rl_amd.RL_OK, rl_amd.REGION_SLOTS)    # region 0 is now full
    assert F.put_keys(rest) == (rl_amd.RL_E_CAPACITY, r1.size)
    assert F.copy_keys(r1).tobytes() == imgs[~in0].tobytes()
    assert F.copy_keys(r0).shape[0] == rl_amd.REGION_SLOTS
    assert F.put_keys(fill[:3]) == (rl_amd.RL_OK, 3)                  # replacing needs no free slot
    assert F.limiter_slots(0) == rl_amd.MIN_REGIONS * rl_amd.REGION_SLOTS
    G.close()
    F.close()


def test_calls_leave_stats_and_status_alone():
    """(j) None of the three calls changes a batch statistic or the status rl_last_status
    reports, nor collects it."""
    A, B = make(), make()
    keys = region_keys(0, 1, 40)
    n = keys.size
    permits = np.ones(n, np.int32)
    permits[3] = 0                                                    # one invalid request
    a, r, t, st = A.execute(keys, permits, np.full(n, T0 * NS, np.int64), np.zeros(n, np.uint16),
                            np.zeros(n, np.uint8))
    assert st == rl_amd.RL_E_INVALID_REQUEST
    stats = A.stats()
    imgs = A.copy_keys(keys)
    assert imgs.shape[0] == n - 1
    assert A.put_keys(imgs) == (rl_amd.RL_OK, n - 1)                  # onto itself: replaces
    assert A.copy_keys(keys).tobytes() == imgs.tobytes()
    assert A.drop_keys(keys[::2]) == keys[::2].size                   # (the invalid one is keys[3])
    assert A.stats() == stats
    assert A.last_status() == rl_amd.RL_E_INVALID_REQUEST
    assert B.put_keys(imgs) == (rl_amd.RL_OK, n - 1)
    assert B.last_status() == rl_amd.RL_OK and B.stats()["n"] == 0
    # argument errors on a live engine: an unknown limiter, too many keys
    bad = imgs[:2].copy()
    bad["limiter"][1] = len(LIMS)
    with pytest.raises(rl_amd.RlError) as ei:
        B.put_keys(bad)
    assert ei.value.status == rl_amd.RL_E_INVALID_ARG
    with pytest.raises(rl_amd.RlError):
        B.copy_keys(np.zeros(rl_amd.MOVE_KEYS_MAX + 1, np.uint64))
    assert B.copy_keys(np.zeros(0, np.uint64)).shape[0] == 0
    assert B.drop_keys(np.zeros(0, np.uint64)) == 0
    assert B.put_keys(imgs[:0]) == (rl_amd.RL_OK, 0)
    A.close()
    B.close()
