"""Table shrink (rl_shrink_plan / rl_shrink_limiter): a limiter's table is halved in place as often
as its live keys allow, every kept slot carried bit for bit (the local-cache word included), dead
slots and tombstones left behind, and every later batch decides exactly as the oracle does.

The limiter set is test_gpu_growth.py's: a token bucket, a sliding window, and a sliding window
with a 40 ms local cache. Every limiter starts at 8 regions and is grown to 64 (6 region bits)
before the first batch. shard_count is 1, so key hash h lies in region mix64(h) >> (64 - k) of a
table with k region bits, at home slot mix64(h) & 0xFC, and the plan's numbers can be computed
in numpy. A key keeps its limiter (mix64(h) % 3), as in test_gpu_growth.py.
"""
import ctypes

import numpy as np
import pytest

import rl_amd
from oracle.coracle import COracle
from test_gpu_growth import LIMS
from test_gpu_parity import NS, T0, assert_same

pytestmark = pytest.mark.gpu

K = 6                                                # region bits of every table at the start
SLOTS = (1 << K) * rl_amd.REGION_SLOTS
NL = len(LIMS)
IMG = rl_amd.KEY_IMAGE_DTYPE
TB_TTL = 2 * LIMS[0][2]                              # a bucket lives two windows after its refill


def engine(**kw):
    kw.setdefault("max_batch", 1 << 16)
    e = rl_amd.Engine(capacity=1, **kw)
    for l in LIMS:
        e.add_limiter(l[0], l[1], l[2], l[3], capacity=l[4], local_cache_ttl_ms=l[5])
    for li in range(NL):
        assert e.limiter_slots(li) == rl_amd.MIN_REGIONS * rl_amd.REGION_SLOTS
        e.grow_limiter(li, SLOTS // 2)
        assert e.limiter_slots(li) == SLOTS
    return e


def make_keys(lo, n):
    return rl_amd.mix64(np.arange(lo, lo + n, dtype=np.uint64) + np.uint64(11 << 40))


def lim_of(keys):
    return (rl_amd.mix64(keys) % np.uint64(NL)).astype(np.uint16)


def region_of(keys, bits):
    return (rl_amd.mix64(keys) >> np.uint64(64 - bits)).astype(np.int64)


def requests(rng, keys, t_ms, reps, span_ms=300):
    """Every key `reps` times in random order, 1 or 2 permits, times ascending over the span."""
    k = np.repeat(np.asarray(keys, np.uint64), reps)
    k = k[rng.permutation(k.size)]
    now = (t_ms * NS + np.sort(rng.integers(0, span_ms * NS, k.size))).astype(np.int64)
    return k, rng.integers(1, 3, k.size).astype(np.int32), now, lim_of(k)


def run(e, o, req, what, ops=None):
    a, r, tok, st = e.execute(*req, ops)
    assert st == rl_amd.RL_OK, (what, rl_amd.strerror(st))
    assert_same((a, r, tok), o.run(*req, ops), what)


def fullest_of(keys, bits=K):
    """fullest[i] of a table of 2^bits regions that holds exactly `keys`."""
    return [int(np.bincount(region_of(keys, bits - i), minlength=1 << (bits - i)).max())
            for i in range(bits - 3 + 1)]


def rule(fullest, slots, min_keys=0):
    """The halvings rule of include/rl_engine.h, written out (shard_count 1)."""
    j = 0
    for i in range(1, len(fullest)):
        if fullest[i] <= 104 and (slots >> i) >= max(2 * min_keys, 8 * 256):
            j = i
    return j


def images(e, li):
    parts = list(e.snapshot(li, chunk=1 << 14))
    return np.concatenate(parts) if parts else np.zeros(0, IMG)


def by_key(imgs):
    return imgs[np.argsort(imgs["key_hash"], kind="stable")]


def exported(e, at):
    return np.sort(e.export_state(at), order=["limiter", "key_hash", "kind", "window_start_ms"])


def test_plan_is_exact_and_only_reads():
    rng = np.random.default_rng(31)
    e, o = engine(), COracle(LIMS)
    keys = make_keys(0, 900)
    run(e, o, requests(rng, keys, T0, 3), "batch 1")
    at = T0 * NS                                     # nothing has expired
    stats, status = e.stats(), e.last_status()
    for li in range(NL):
        mine = keys[lim_of(keys) == li]
        assert 250 < mine.size < 350
        before = (e.limiter_slots(li), e.limiter_usage(li, at), images(e, li).tobytes())
        want = fullest_of(mine)
        p = e.shrink_plan(li, at)
        print(li, p, want)
        assert p["levels"] == K - 3 + 1 and p["fullest"] == want
        assert p["kept"] == mine.size == p["used_before"]
        assert p["slots_before"] == SLOTS and p["halvings"] == rule(want, SLOTS) == 3
        assert p["slots_after"] == SLOTS >> 3
        # min_keys stops it early: 4096 keys need 8192 slots, 4097 more than that
        assert e.shrink_plan(li, at, min_keys=4096)["halvings"] == rule(want, SLOTS, 4096) == 1
        assert e.shrink_plan(li, at, min_keys=4097)["halvings"] == rule(want, SLOTS, 4097) == 0
        # a later now: the sliding windows and the cache entries have run out, the buckets not
        late = e.shrink_plan(li, (T0 + TB_TTL) * NS)
        assert late["kept"] == (mine.size if LIMS[li][0] == rl_amd.TB else 0)
        assert late["used_before"] == mine.size
        assert (e.limiter_slots(li), e.limiter_usage(li, at), images(e, li).tobytes()) == before
    assert e.stats() == stats and e.last_status() == status
    # argument checks on a live engine: nothing is written
    r = rl_amd.ShrinkReport()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    raw = bytes(r)
    L = rl_amd.lib()
    assert L.rl_shrink_plan(e.handle, NL, at, 0, ctypes.byref(r)) == rl_amd.RL_E_INVALID_ARG
    assert L.rl_shrink_plan(e.handle, 0, at, 0, None) == rl_amd.RL_E_INVALID_ARG
    assert L.rl_shrink_limiter(e.handle, NL, at, 0, ctypes.byref(r)) == rl_amd.RL_E_INVALID_ARG
    assert bytes(r) == raw and [e.limiter_slots(li) for li in range(NL)] == [SLOTS] * NL
    e.close()
    o.close()


def test_shrink_keeps_the_keyspace():
    rng = np.random.default_rng(32)
    e, u, o = engine(), engine(), COracle(LIMS)      # u: the same engine, never shrunk
    keys = make_keys(0, 900)
    req1 = requests(rng, keys, T0, 5)                # (the fourth allow of a key sets its cache entry)
    run(e, o, req1, "batch 1")
    assert u.execute(*req1)[3] == rl_amd.RL_OK
    at = T0 * NS                                     # everything is live
    state = exported(e, int(req1[2][-1]))
    assert state.size > 0
    snaps = [images(e, li) for li in range(NL)]
    for li in range(NL):
        plan = e.shrink_plan(li, at)
        r = e.shrink_limiter(li, at)
        assert r == plan and r["halvings"] == 3
        assert e.limiter_slots(li) == r["slots_before"] >> r["halvings"] == r["slots_after"]
        assert e.limiter_usage(li, at)["used_slots"] == r["kept"] == snaps[li].shape[0]
        now_imgs = images(e, li)
        assert by_key(now_imgs).tobytes() == by_key(snaps[li]).tobytes()       # cache_word included
        assert np.all(np.diff(region_of(now_imgs["key_hash"], K - 3)) >= 0)
        for other in range(li + 1, NL):              # the later limiters' tables: as they were
            assert e.limiter_slots(other) == SLOTS
            assert images(e, other).tobytes() == snaps[other].tobytes()
    assert snaps[2]["cache_word"].any()
    assert np.array_equal(exported(e, int(req1[2][-1])), state)
    assert e.stats()["table_grows"] == u.stats()["table_grows"]
    # the next batch: old and new keys under all three limiters, and acquires on keys that the
    # local cache still blocks (their cache word lies beyond the request's time)
    t2 = T0 + 290
    req2 = requests(rng, np.concatenate([keys[::2], make_keys(900, 400)]), t2, 2, span_ms=40)
    block = dict(zip(snaps[2]["key_hash"].tolist(), snaps[2]["cache_word"].tolist()))
    hit = [i for i in range(req2[0].size)
           if req2[3][i] == 2 and block.get(int(req2[0][i]), 0) > int(req2[2][i]) // NS]
    print("blocked acquires:", len(hit))
    assert len(hit) > 0 and set(req2[3].tolist()) == {0, 1, 2}
    got = e.execute(*req2)
    assert got[3] == rl_amd.RL_OK
    assert_same(got[:3], o.run(*req2), "batch 2 vs oracle")
    assert_same(got[:3], u.execute(*req2)[:3], "batch 2 vs the unshrunk engine")
    assert not got[0][hit].any()                     # (the blocked acquires were denied)
    for x in (e, u, o):
        x.close()


def test_shrink_stops_by_fill():
    rng = np.random.default_rng(33)
    e, o = engine(), COracle(LIMS)
    keys = make_keys(0, 3600)
    run(e, o, requests(rng, keys, T0, 1), "batch 1")
    assert [e.limiter_slots(li) for li in range(NL)] == [SLOTS] * NL          # nothing grew
    for li in range(NL):
        want = fullest_of(keys[lim_of(keys) == li])
        j = rule(want, SLOTS)
        print(li, want, j)
        assert 0 < j < K - 3                         # strictly between "no change" and 8 regions
        assert want[j] <= 104 < want[j + 1]
        r = e.shrink_limiter(li, T0 * NS)
        assert r["fullest"] == want and r["halvings"] == j
        assert e.limiter_slots(li) == SLOTS >> j
    run(e, o, requests(rng, np.concatenate([keys[::3], make_keys(3600, 200)]), T0 + 300, 2), "batch 2")
    e.close()
    o.close()


def test_a_table_at_design_load_is_left_alone():
    rng = np.random.default_rng(34)
    e, o = engine(), COracle(LIMS)
    keys = make_keys(0, NL * (1 << K) * 128)         # ~128 keys per region
    run(e, o, requests(rng, keys, T0, 1), "batch 1")
    assert [e.limiter_slots(li) for li in range(NL)] == [SLOTS] * NL
    stats = e.stats()
    for li in range(NL):
        want = fullest_of(keys[lim_of(keys) == li])
        assert want[0] > 104 and rule(want, SLOTS) == 0
        before = images(e, li)
        assert before.shape[0] > 7000
        st = rl_amd.lib().rl_shrink_limiter(e.handle, li, T0 * NS, 0, None)   # the report is optional
        assert st == rl_amd.RL_OK
        r = e.shrink_limiter(li, T0 * NS)
        assert r["halvings"] == 0 and r["slots_after"] == r["slots_before"] == SLOTS
        assert r["fullest"] == want
        assert images(e, li).tobytes() == before.tobytes()                     # the same order too
        assert e.limiter_slots(li) == SLOTS
    assert e.stats() == stats
    e.close()
    o.close()


def spread_keys(n_each, groups):
    """`groups` disjoint key sets, n_each keys per limiter each, no two keys of one limiter in
    the same 4-slot home bucket of the 64-region table: every key sits in its home slot and no
    insert probes into (or reuses) another key's slot."""
    cand = make_keys(0, 40_000)
    tag = rl_amd.mix64(cand)
    bucket = (lim_of(cand).astype(np.uint64) << np.uint64(32)) | \
        ((tag >> np.uint64(64 - K)) << np.uint64(8)) | (tag & np.uint64(0xFC))
    _, first = np.unique(bucket, return_index=True)
    cand = cand[np.sort(first)]
    lim = lim_of(cand)
    out = []
    for g in range(groups):
        out.append(np.concatenate([cand[lim == li][g * n_each:(g + 1) * n_each] for li in range(NL)]))
        assert out[-1].size == NL * n_each
    return out


def test_shrink_sweeps():
    rng = np.random.default_rng(35)
    e, o = engine(), COracle(LIMS)
    A, B = spread_keys(100, 2)
    run(e, o, requests(rng, A, T0, 2), "group A")
    t1 = T0 + TB_TTL + 400                           # every key of A is dead from here on
    run(e, o, requests(rng, B, t1, 2), "group B")
    gone = np.concatenate([B[lim_of(B) == li][:5] for li in range(NL)])
    ops = np.full(gone.size, rl_amd.OP_RESET, np.uint8)
    run(e, o, (gone, np.ones(gone.size, np.int32), np.full(gone.size, (t1 + 300) * NS, np.int64),
               lim_of(gone)), "resets", ops)
    at = (t1 + 400) * NS                             # (past the cache entries of group B)
    for li in range(NL):
        census = e.limiter_usage(li, at)
        r = e.shrink_limiter(li, at)
        print(li, r, census["used_slots"], census["live_keys"])
        assert r["kept"] == 100 - 5 == census["live_keys"]
        assert r["used_before"] - r["kept"] == 100 + 5           # A's dead slots and the tombstones
        assert r["used_before"] == census["used_slots"]
        assert r["halvings"] == 3 and e.limiter_slots(li) == SLOTS >> 3
        after = e.limiter_usage(li, at)
        assert after["used_slots"] == after["live_keys"] == r["kept"]
        kept = images(e, li)["key_hash"]
        assert set(kept.tolist()) == set(B[lim_of(B) == li][5:].tolist())
    # A's keys start fresh, B's go on, the reset ones start fresh too
    run(e, o, requests(rng, np.concatenate([A, B]), t1 + 400, 2), "A and B after the shrink")
    e.close()
    o.close()


def test_a_shrunk_table_grows_again():
    rng = np.random.default_rng(36)
    e, o = engine(), COracle(LIMS)
    known = 300
    run(e, o, requests(rng, make_keys(0, known), T0, 2), "batch 1")
    for li in range(NL):
        assert e.shrink_limiter(li, T0 * NS)["halvings"] == 3
    small = rl_amd.MIN_REGIONS * rl_amd.REGION_SLOTS
    assert [e.limiter_slots(li) for li in range(NL)] == [small] * NL
    grows0, t = e.stats()["table_grows"], T0 + 250
    for b in range(14):
        # each batch brings about 1/16 of the smallest current table as new keys: a region past
        # 208 keys flags growth well before one batch's share (16 per region) can fill it
        fresh = min(e.limiter_slots(li) for li in range(NL)) // 16 * NL
        old = make_keys(0, known)[rng.integers(0, known, 2000)]
        req = requests(rng, np.concatenate([make_keys(known, fresh), old]), t, 1)
        known += fresh
        t += 250
        run(e, o, req, f"batch {b + 2}")
    st = e.stats()
    assert st["table_grows"] > grows0 and st["capacity_errors"] == 0
    assert all(e.limiter_slots(li) > small for li in range(NL))
    e.close()
    o.close()


def test_shrink_between_two_pipelined_batches():
    import torch
    rng = np.random.default_rng(37)
    e, o = engine(pipeline=True), COracle(LIMS)
    keys = make_keys(0, 900)
    reqs = [requests(rng, keys, T0, 2), requests(rng, np.concatenate([keys[::2], make_keys(900, 300)]),
                                                 T0 + 300, 2)]
    dev, outs = [], []
    for k, p, t, l in reqs:
        dev.append([torch.from_numpy(np.ascontiguousarray(x)).cuda()
                    for x in (k.view(np.int64), p, t, l.view(np.int16))])
        outs.append((torch.empty(k.size, dtype=torch.uint8, device="cuda"),
                     torch.empty(k.size, dtype=torch.int64, device="cuda"),
                     torch.empty(k.size, dtype=torch.float64, device="cuda")))
    torch.cuda.synchronize()
    e.execute_device(reqs[0][0].size, *dev[0], None, *outs[0])
    reports = [e.shrink_limiter(li, T0 * NS) for li in range(NL)]   # behind batch 1, no sync before
    e.execute_device(reqs[1][0].size, *dev[1], None, *outs[1])
    e.sync()
    assert e.last_status() == rl_amd.RL_OK
    for li, r in enumerate(reports):
        assert r["kept"] == int(np.sum(lim_of(keys) == li)) and r["halvings"] == 3
        assert e.limiter_slots(li) == SLOTS >> 3
    for i, req in enumerate(reqs):
        got = tuple(x.cpu().numpy() for x in outs[i])
        assert_same(got, o.run(*req), f"pipelined batch {i + 1}")
    e.close()
    o.close()
