"""Mixed operations and retry-after queries through CRouter (rl_router_execute,
rl_router_retry_after): two gloo ranks share the GPU over the host transport. Every step's
decisions must equal the oracle's on the global stream (COracle.run with ops), and every wait
what an unsharded rl_amd.Engine in the parent, fed the same stream, answers for the same
queries."""
import datetime
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

NS = 1_000_000
T0 = 1_700_000_000_000
LIMS = [[1, 50, 60000, 10.0], [0, 30, 5000, 0.0]]       # token bucket, sliding window
WORLD, STEPS, N, NQ = 2, 3, 5000, 700
# A rank asks about its own slice after the step, so a query's now lies up to a step's span (7 s)
# before the end of the stream; split rounds are separate engine batches with later earliest
# requests than the parent engine's one batch per step. rl_opts.max_skew_ms covers timestamps
# that lag behind earlier batches; the workers' engines and the parent's get the same allowance.
SKEW_MS = 10_000


def _trace():
    import rl_amd
    rng = np.random.default_rng(23)
    total = STEPS * WORLD * N
    ranks = np.minimum(rng.zipf(1.2, total), 5000) - 1
    keys = rl_amd.mix64(ranks.astype(np.uint64))
    permits = rng.integers(1, 5, total).astype(np.int32)
    t = np.sort(rng.integers(0, 20_000 * NS, total))
    lim = (ranks % 2).astype(np.uint16)
    ops = rng.choice(np.array([0, 1, 2], np.uint8), total, p=[0.90, 0.07, 0.03])
    ops[11::997] = 3                                     # invalid operations and limiter ids
    lim[13::997] = 0x4001
    permits[17::997] = 0
    return keys, permits, (T0 * NS + t).astype(np.int64), lim, ops


def _queries(rank):
    """The second query of a rank: rank 0 asks nothing; rank 1 seen and unseen keys, permits 0
    and beyond every maximum, an unknown limiter; every third query skipped."""
    import rl_amd
    if rank == 0:
        z = np.zeros(0, np.int64)
        return z.astype(np.uint64), z.astype(np.int32), z, z.astype(np.uint16), z.astype(np.uint8)
    i = np.arange(NQ)
    keys = rl_amd.mix64((i % 40).astype(np.uint64))
    keys[1::5] = rl_amd.mix64((i[1::5] + 1_000_000).astype(np.uint64))
    permits = (1 + i % 4).astype(np.int32)
    permits[2::7] = 0
    permits[3::7] = 1000
    lim = (i % 2).astype(np.uint16)
    lim[4::11] = 300
    now = ((T0 + 20_000 + i % 500) * NS).astype(np.int64)
    return keys, permits, now, lim, (i % 3 == 0).astype(np.uint8)


def _worker(rank, port, out):
    import rl_amd
    from rl_amd.capi_router import CRouter
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD,
                            timeout=datetime.timedelta(seconds=120))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    eng = rl_amd.Engine(device=0, max_batch=WORLD * N, capacity=1 << 14, shard_index=rank,
                        shard_count=WORLD, max_skew_ms=SKEW_MS)
    for l in LIMS:
        eng.add_limiter(*l)
    router = CRouter(eng, WORLD, rank, N, transport="host", device=0, recv_cap=N + 1500)
    keys, permits, now, lim, ops = _trace()

    def up(x, view=None):
        x = np.ascontiguousarray(x)
        return torch.from_numpy((x.view(view) if view else x).copy()).to(dev)

    res_a, res_r = [], []
    for s in range(STEPS):
        sl = slice((s * WORLD + rank) * N, (s * WORLD + rank + 1) * N)
        k, p, t = up(keys[sl], np.int64), up(permits[sl]), up(now[sl])
        li, o = up(lim[sl], np.int16), up(ops[sl])
        a = torch.empty(N, dtype=torch.uint8, device=dev)
        r = torch.empty(N, dtype=torch.int64, device=dev)
        router.execute(N, k, p, t, li, o, a, r)
        torch.cuda.synchronize()
        res_a.append(a.cpu().numpy())
        res_r.append(r.cpu().numpy())
    # the last step's own arrays and its allowed output, then a second query of another shape
    before = (eng.stats(), router.stats())
    w1 = torch.full((N,), 99, dtype=torch.int64, device=dev)
    router.retry_after(N, k, p, t, li, a, w1)
    qk, qp, qt, ql, qs = _queries(rank)
    n2 = qk.size
    w2 = torch.full((max(n2, 1),), 99, dtype=torch.int64, device=dev)
    if n2:
        router.retry_after(n2, up(qk, np.int64), up(qp), up(qt), up(ql, np.int16), up(qs), w2)
    else:
        router.retry_after(0, None, None, None, w2, None, None)      # limiter non-NULL, as rank 1's
    after = (eng.stats(), router.stats())
    for f in ("steps", "rounds", "split_steps", "max_recv"):
        assert after[1][f] == before[1][f], f
    assert after[0] == before[0]
    assert router.finish() == rl_amd.RL_E_INVALID_REQUEST
    router.close()
    np.savez(f"{out}.{rank}.npz", a=np.concatenate(res_a), r=np.concatenate(res_r),
             w1=w1.cpu().numpy(), w2=w2.cpu().numpy()[:n2])
    dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_ops_and_waits_through_two_ranks(tmp_path):
    import rl_amd
    from oracle.coracle import COracle
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "p")
    ctx = mp.spawn(_worker, args=(port, out), nprocs=WORLD, join=False)
    deadline = time.monotonic() + 200
    while not ctx.join(timeout=5):                       # re-raises a worker's failure
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the router workers did not finish in time")
    keys, permits, now, lim, ops = _trace()
    wa, wr, _, _ = COracle(LIMS).run(keys, permits, now, lim, ops=ops, want_tokens=False)
    assert 0 < wa.sum() < wa.size
    got = [np.load(f"{out}.{rank}.npz") for rank in range(WORLD)]
    for rank in range(WORLD):
        for st in range(STEPS):
            sl = slice((st * WORLD + rank) * N, (st * WORLD + rank + 1) * N)
            assert np.array_equal(got[rank]["a"][st * N:(st + 1) * N], wa[sl]), (rank, st)
            assert np.array_equal(got[rank]["r"][st * N:(st + 1) * N], wr[sl]), (rank, st)
    # the waits: one unsharded engine fed the same stream
    eng = rl_amd.Engine(device=0, max_batch=STEPS * WORLD * N, capacity=1 << 14, max_skew_ms=SKEW_MS)
    for l in LIMS:
        eng.add_limiter(*l)
    for st in range(STEPS):
        sl = slice(st * WORLD * N, (st + 1) * WORLD * N)
        a, r, _, status = eng.execute(keys[sl], permits[sl], now[sl], lim[sl], ops[sl], want_tokens=False)
        assert np.array_equal(a, wa[sl]) and np.array_equal(r, wr[sl])
    some_wait = 0
    for rank in range(WORLD):
        sl = slice(((STEPS - 1) * WORLD + rank) * N, ((STEPS - 1) * WORLD + rank + 1) * N)
        want, _ = eng.retry_after(lim[sl], keys[sl], permits[sl], now[sl], skip=wa[sl])
        assert np.array_equal(got[rank]["w1"], want), rank
        some_wait += int((want > 0).sum())
        qk, qp, qt, ql, qs = _queries(rank)
        if qk.size:
            want2, _ = eng.retry_after(ql, qk, qp, qt, skip=qs)
            assert np.array_equal(got[rank]["w2"], want2), rank
            assert (want2 == rl_amd.RETRY_NEVER).any() and (want2 == rl_amd.RETRY_INVALID).any()
        else:
            assert got[rank]["w2"].size == 0
    assert some_wait > 0
