"""Long probe chains through both users of the quad probe (csrc/rl_table.hpp): retry-after and
key migration, with the census and the state export beside them.

Two engines get the same limiter and the same requests for the same K keys. Engine N is sized
as usual, so nearly every probe chain is one 4-slot bucket. Engine F is a fixed-capacity table
whose keys' tags all fall into region 0 (256 slots): K = 200 keys there are a load of 0.78, at
which a linear probe regularly crosses buckets and wraps the region. Key hash 0 (tag 0) is among
the keys. Whatever is asked of the two tables afterwards has to come out the same.
"""
import numpy as np
import pytest

import rl_amd

pytestmark = pytest.mark.gpu

NS = 1_000_000
T0 = 1_700_000_000_000                     # a multiple of the window
W = 4000
K, ABSENT = 200, 56
BITS = rl_amd.MIN_REGIONS.bit_length() - 1
LIMS = {"sw": dict(algo=rl_amd.SW, max_permits=6, window_ms=W),
        "tb": dict(algo=rl_amd.TB, max_permits=10, window_ms=W, refill_per_s=2.5)}
# inside the second window, at its edge, past every TTL (both algorithms: 2 w after the last write)
NOWS = (T0 + W + 1500, T0 + 2 * W, T0 + 10 * W)


def region0_keys():
    """Key 0 and K + ABSENT - 1 more keys whose tags fall into region 0 of the smallest table."""
    cand = np.arange(0, 200_000, dtype=np.uint64)
    keys = cand[rl_amd.mix64(cand) >> np.uint64(64 - BITS) == 0][:K + ABSENT]
    assert keys.size == K + ABSENT and keys[0] == 0
    return keys[:K], keys[K:]


def batches(present):
    """Every key in the first window and again in the second (both buckets get requests)."""
    rng = np.random.default_rng(20)
    out = []
    for n, lo, hi in ((3 * K, T0, T0 + W), (2 * K, T0 + W, T0 + W + 1000)):
        keys = np.concatenate([present, present[rng.integers(0, K, n - K)]])
        now = np.sort(rng.integers(lo, hi, n))
        keys = keys[rng.permutation(n)]
        out.append((keys, rng.integers(1, 4, n).astype(np.int32), (now * NS).astype(np.int64),
                    np.zeros(n, np.uint16), np.zeros(n, np.uint8)))
    return out


def images(e, keys):
    im = e.copy_keys(keys)
    return [(int(x["limiter"]), int(x["key_hash"]), *map(int, x["word"]), int(x["cache_word"])) for x in im]


def same_answers(F, N, keys, permits):
    """Retry-after at the three instants and the copy of all 256 keys: F against N. Returns the
    waits at the first instant and the keys that have an image."""
    waits = []
    for now in NOWS:
        wf, sf = F.retry_after(0, keys, permits, now * NS)
        wn, sn = N.retry_after(0, keys, permits, now * NS)
        assert sf == sn == rl_amd.RL_OK
        assert np.array_equal(wf, wn), f"now {now}: {np.nonzero(wf != wn)[0][:8]}"
        waits.append(wf)
    imf, imn = images(F, keys), images(N, keys)
    assert imf == imn
    return waits[0], {i[1] for i in imf}


def same_census(F, N):
    uf, un = F.limiter_usage(0, NOWS[0] * NS), N.limiter_usage(0, NOWS[0] * NS)
    for f in ("live_keys", "redis_keys", "used_permits", "hist"):
        assert uf[f] == un[f], f
    ef, en = F.export_state(NOWS[0] * NS), N.export_state(NOWS[0] * NS)
    assert ef.shape == en.shape and ef.tobytes() == en.tobytes()
    return uf, ef


@pytest.mark.parametrize("algo", ["sw", "tb"])
def test_long_chains_answer_as_short_ones(algo):
    present, absent = region0_keys()
    allkeys = np.concatenate([present, absent])
    F = rl_amd.Engine(max_batch=1 << 16, capacity=1, fixed_capacity=True)
    N = rl_amd.Engine(max_batch=1 << 16, capacity=1 << 16)
    F.add_limiter(capacity=1, **LIMS[algo])
    N.add_limiter(**LIMS[algo])
    assert F.limiter_slots(0) == rl_amd.MIN_REGIONS * rl_amd.REGION_SLOTS < N.limiter_slots(0)
    for b in batches(present):
        af, rf, _, sf = F.execute(*b)
        an, rn, _, sn = N.execute(*b)
        assert sf == sn == rl_amd.RL_OK                       # the region took all K keys
        assert np.array_equal(af, an) and np.array_equal(rf, rn)
    assert F.limiter_slots(0) == rl_amd.MIN_REGIONS * rl_amd.REGION_SLOTS
    permits = np.random.default_rng(21).integers(1, LIMS[algo]["max_permits"] + 1, allkeys.size).astype(np.int32)
    # 1, 2: retry-after and copy
    wait, found = same_answers(F, N, allkeys, permits)
    assert found == set(map(int, present))
    assert (wait[:K] > 0).any() and (wait[K:] == 0).all()     # denials exist; absent keys pass
    # 4: census and export (before and after the drop)
    use, ent = same_census(F, N)
    assert 0 < use["live_keys"] == np.unique(ent["key_hash"]).size and np.isin(ent["key_hash"], present).all()
    # 3: tombstones inside the chains
    dropped = present[::3]
    assert F.drop_keys(dropped) == N.drop_keys(dropped) == dropped.size
    wait, found = same_answers(F, N, allkeys, permits)
    assert found == set(map(int, present)) - set(map(int, dropped))
    assert images(F, dropped) == images(N, dropped) == []
    assert (wait[:K][::3] == 0).all()                         # a dropped key reads as absent
    use, ent = same_census(F, N)
    assert use["live_keys"] == np.unique(ent["key_hash"]).size and not np.isin(ent["key_hash"], dropped).any()
    F.close()
    N.close()
