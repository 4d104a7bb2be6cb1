"""The routing kernels behind rl_router_execute / rl_router_retry_after, one by one on the GPU:
the owner partition restricted to the non-skipped requests (rl_route_partition_skip_device),
the ops column (rl_route_fold_ops / rl_route_unfold_ops) and the wait unpack
(rl_route_unpack_wait). Expected values come from numpy and rl_amd.owner_of."""
import numpy as np
import pytest
import torch

import rl_amd

pytestmark = pytest.mark.gpu

TILE = 65536                                    # requests per partition tile (kTile)
SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1]
DEV = "cuda"


def _dev(a):
    """numpy -> device tensor of the same bytes (torch has no unsigned 16 / 32 / 64-bit kernels)."""
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype)).copy()).to(DEV)


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


_engines = {}


def _engine(shards):
    """One engine per shard count, with a few keys in an installed directory."""
    if shards not in _engines:
        e = rl_amd.Engine(device=0, max_batch=1 << 12, capacity=1 << 10, shard_index=0, shard_count=shards)
        e.add_limiter(rl_amd.TB, 50, 60_000, 10.0)
        dk = rl_amd.mix64(np.arange(1, 9, dtype=np.uint64))
        do = (np.arange(8, dtype=np.uint32) * 3 + 1) % shards
        e.set_owner_directory(dk, do)
        _engines[shards] = (e, dk, do)
    return _engines[shards]


def _keys(n, dir_keys):
    rng = np.random.default_rng(n + 5)
    k = rl_amd.mix64(rng.integers(0, 4000, n).astype(np.uint64) + np.uint64(100))
    if n:
        hot = rng.random(n) < 0.2                 # a fifth of the requests hit the directory's keys
        k[hot] = dir_keys[rng.integers(0, len(dir_keys), int(hot.sum()))]
    return k


def _owners(keys, shards, dir_keys, dir_owner):
    own = rl_amd.owner_of(keys, shards).astype(np.uint32)
    for k, o in zip(dir_keys, dir_owner):
        own[keys == k] = o
    return own


@pytest.mark.parametrize("shards", [1, 2, 4, 8, 16, 32, 64])
@pytest.mark.parametrize("n", SIZES)
def test_skip_partition(n, shards):
    eng, dk, do = _engine(shards)
    keys = _keys(n, dk)
    own = _owners(keys, shards, dk, do)
    if shards > 1 and n > 1000:
        assert len(set(own.tolist())) == shards
    rng = np.random.default_rng(n * 8 + shards)
    kd = _dev(keys) if n else torch.zeros(1, dtype=torch.int64, device=DEV)
    stride = 3
    for share in (None, 0.0, 0.5, 1.0):
        skip = None if share is None else (rng.random(n) < share).astype(np.uint8) * np.uint8(1 + (n % 200))
        live = np.arange(n) if skip is None else np.nonzero(skip == 0)[0]
        want = live[np.argsort(own[live], kind="stable")].astype(np.uint32)
        perm = torch.full((max(n, 1),), -1, dtype=torch.int32, device=DEV)
        counts = torch.full((shards * stride,), -7, dtype=torch.int64, device=DEV)
        sd = None if skip is None else (_dev(skip) if n else torch.zeros(1, dtype=torch.uint8, device=DEV))
        eng.route_partition_skip_device(n, kd, sd, perm, shards, counts, stride)
        torch.cuda.synchronize()
        c = counts.cpu().numpy().reshape(shards, stride)
        assert np.array_equal(c[:, 0], np.bincount(own[live], minlength=shards)), (n, shards, share)
        assert np.all(c[:, 1:] == -7)
        got = _host(perm, np.uint32)
        assert int(c[:, 0].sum()) == live.size
        assert np.array_equal(got[:live.size], want), (n, shards, share)
        assert np.all(got[live.size:] == 0xFFFFFFFF)          # the tail is not written
        if skip is None:                                      # NULL skip is the plain partition
            perm2 = torch.full((max(n, 1),), -1, dtype=torch.int32, device=DEV)
            counts2 = torch.full((shards * stride,), -7, dtype=torch.int64, device=DEV)
            eng.route_partition_device(n, kd, perm2, shards, counts2, stride)
            torch.cuda.synchronize()
            assert torch.equal(perm, perm2) and torch.equal(counts, counts2)


LIMS = [0, 1, 254, 255, 0x3FFE, 0x3FFF, 0x4000, 0x4001, 0xFFFF]
OPS = [0, 1, 2, 3, 255]


@pytest.mark.parametrize("n", [0, 1, 257, 5000])
def test_fold_and_unfold_ops(n):
    eng, _, _ = _engine(1)
    rng = np.random.default_rng(n)
    pairs = np.array([(l, o) for l in LIMS for o in OPS], np.uint32)
    pick = np.arange(n) % len(pairs) if n >= len(pairs) else rng.integers(0, len(pairs), n)
    lim = pairs[pick, 0].astype(np.uint16)
    op = pairs[pick, 1].astype(np.uint8)
    perm = rng.permutation(n).astype(np.uint32)
    m = max(n, 1)
    pd = _dev(perm) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    ld = _dev(lim) if n else torch.zeros(1, dtype=torch.int16, device=DEV)
    od = _dev(op) if n else torch.zeros(1, dtype=torch.uint8, device=DEV)
    for use_lim, use_op in ((True, True), (False, True), (True, False), (False, False)):
        l = lim[perm].astype(np.uint32) if use_lim else np.zeros(n, np.uint32)
        o = op[perm].astype(np.uint32) if use_op else np.zeros(n, np.uint32)
        want = (np.minimum(l, 0x3FFF) | (np.minimum(o, 3) << 14)).astype(np.uint16)
        col = torch.full((m,), -1, dtype=torch.int16, device=DEV)
        eng.route_fold_ops(n, pd, ld if use_lim else None, od if use_op else None, col)
        torch.cuda.synchronize()
        assert np.array_equal(_host(col, np.uint16)[:n], want), (n, use_lim, use_op)
        # an id past 0x3FFF never aliases a valid limiter, an op past 2 never a valid op
        assert np.all((want & 0x3FFF)[l > 255] > 255) and np.all((want >> 14)[o > 2] == 3)
        # unfold into separate arrays, then in place
        lo = torch.full((m,), -1, dtype=torch.int16, device=DEV)
        oo = torch.full((m,), 77, dtype=torch.uint8, device=DEV)
        eng.route_unfold_ops(n, col, lo, oo)
        torch.cuda.synchronize()
        assert np.array_equal(_host(lo, np.uint16)[:n], want & 0x3FFF)
        assert np.array_equal(oo.cpu().numpy()[:n], (want >> 14).astype(np.uint8))
        assert np.array_equal(_host(col, np.uint16)[:n], want)           # the source is intact
        oo2 = torch.full((m,), 77, dtype=torch.uint8, device=DEV)
        eng.route_unfold_ops(n, col, col, oo2)
        torch.cuda.synchronize()
        assert np.array_equal(_host(col, np.uint16)[:n], want & 0x3FFF)
        assert torch.equal(oo, oo2)
        if n == 0:
            assert int(col[0]) == -1 and int(oo2[0]) == 77


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_unpack_wait(n):
    eng, _, _ = _engine(1)
    rng = np.random.default_rng(n + 1)
    back = rng.integers(-2, 1 << 40, n).astype(np.int64)
    for share in (None, 0.0, 0.5, 1.0):
        skip = None if share is None else (rng.random(n) < share).astype(np.uint8) * np.uint8(3)
        live = np.arange(n) if skip is None else np.nonzero(skip == 0)[0]
        perm = np.full(n, 0xFFFFFFFF, np.uint32)              # past the prefix: not to be read
        perm[:live.size] = rng.permutation(live)
        want = np.zeros(n, np.int64)
        want[perm[:live.size]] = back[:live.size]
        wait = torch.full((n,), 99, dtype=torch.int64, device=DEV)
        eng.route_unpack_wait(n, live.size, _dev(perm), _dev(back), None if skip is None else _dev(skip), wait)
        torch.cuda.synchronize()
        assert np.array_equal(wait.cpu().numpy(), want), (n, share)
    with pytest.raises(rl_amd.RlError):                       # n_live > n
        eng.route_unpack_wait(n, n + 1, _dev(perm), _dev(back), None, wait)
