#!/usr/bin/env python3
"""Time of the key-migration calls and of a directory re-plan on a live router, beside one
router step of the same engines for scale.

engine   rl_copy_keys / rl_put_keys / rl_drop_keys at 1, 1024 and 8192 keys x 1, 2 and 10
         token-bucket limiters: engine A holds every probe key under every limiter among
         `--population` other keys; the images are copied from A, put into an empty engine B and
         dropped from B again. Each call synchronises itself, so it is timed on the host clock
         around the call: after one warm-up, the median of `--reps` repetitions (min, max).
replan   two ranks on this GPU over the host transport (a functional stand-in for RCCL: its
         all-to-alls go through the host, so the exchange part of these times says nothing about
         xGMI), bench.py's zipf_1b trace, `--batch` requests per rank per step: two steps, a
         re-plan of k = 4096 keys from a device sample of the last step (rl_top_keys with
         min_count = 3 included), a step, a re-plan with no candidates (everything goes home), a
         step. The slower rank's time of each is printed, with (placed, moved) of each re-plan.
step     the same first two steps only (no new entry point), to set beside the same two steps
         of another build of the library and package.

usage: tools/migrate_probe.py [--parts engine replan step] [--reps 7] [--batch 1048576]
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

import bench  # noqa: E402
import rl_amd  # noqa: E402

NS = 1_000_000
T0 = 1_700_000_000_000
WORLD = 2


def stats(ms):
    return [round(x, 4) for x in (statistics.median(ms), min(ms), max(ms))]


def engine_case(n_lim, population, reps):
    A = rl_amd.Engine(max_batch=1 << 21, capacity=1 << 20)
    B = rl_amd.Engine(max_batch=1 << 21, capacity=1 << 20)
    for e in (A, B):
        for _ in range(n_lim):
            e.add_limiter(rl_amd.TB, 50, 60_000, 10.0)
    rng = np.random.default_rng(5)
    probe = rng.integers(1, 2**63, 8192, dtype=np.uint64)
    keys = np.concatenate([np.repeat(probe, n_lim), rng.integers(1, 2**63, population, dtype=np.uint64)])
    lim = np.concatenate([np.tile(np.arange(n_lim, dtype=np.uint16), probe.size),
                          rng.integers(0, n_lim, population).astype(np.uint16)])
    n = keys.size
    st = A.execute(keys, np.ones(n, np.int32), np.full(n, T0 * NS, np.int64), lim, None, want_tokens=False)[3]
    assert st == rl_amd.RL_OK, rl_amd.strerror(st)
    out = []
    for nk in (1, 1024, 8192):
        ks = probe[:nk]
        t_copy, t_put, t_drop = [], [], []
        for i in range(reps + 1):                   # the first run warms up
            t0 = time.perf_counter()
            imgs = A.copy_keys(ks)
            t1 = time.perf_counter()
            assert B.put_keys(imgs) == (rl_amd.RL_OK, nk * n_lim)
            t2 = time.perf_counter()
            assert B.drop_keys(ks) == nk * n_lim
            t3 = time.perf_counter()
            if i:
                t_copy.append((t1 - t0) * 1e3)
                t_put.append((t2 - t1) * 1e3)
                t_drop.append((t3 - t2) * 1e3)
        out.append({"limiters": n_lim, "keys": nk, "images": int(imgs.shape[0]), "copy_ms": stats(t_copy),
                    "put_ms": stats(t_put), "drop_ms": stats(t_drop)})
        print(json.dumps(out[-1]), flush=True)
    A.close()
    B.close()
    return out


def _rank(rank, port, n, replan, out):
    from rl_amd.capi_router import CRouter
    cfg = bench.CONFIGS["zipf_1b"]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    torch.cuda.set_device(0)
    eng = rl_amd.Engine(device=0, max_batch=WORLD * n, capacity=1 << 22, shard_index=rank,
                        shard_count=WORLD)
    for l in cfg["limiters"]:
        eng.add_limiter(*l)
    steps = 4
    slices = bench.make_inputs(eng, cfg, n, WORLD, rank, steps, "cuda")
    eng.sync()
    router = CRouter(eng, WORLD, rank, n, transport="host", device=0)
    a = torch.empty(n, dtype=torch.uint8, device="cuda")
    r = torch.empty(n, dtype=torch.int64, device="cuda")
    res = {}

    def timed(name, fn):
        dist.barrier()
        t = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        res[name] = round((time.perf_counter() - t) * 1e3, 3)
        return v

    def step(s):
        k, p, t, li = slices[s]
        router.step(n, k, p, t, li, a, r)

    timed("step0_ms", lambda: step(0))              # (first step: code objects load)
    timed("step1_ms", lambda: step(1))
    if replan:
        res["replan_sampled"] = timed("replan_sampled_ms",
                                      lambda: router.replan_directory_sampled(slices[1][0], 4096, 3))
        timed("step2_ms", lambda: step(2))
        z = np.zeros(0, np.uint64)
        res["replan_clear"] = timed("replan_clear_ms", lambda: router.replan_directory(z, z, 0, 4096))
        timed("step3_ms", lambda: step(3))
    assert router.finish() == rl_amd.RL_OK
    box = [None] * WORLD
    dist.all_gather_object(box, res)
    if rank == 0:
        worst = {k: (max(b[k] for b in box) if k.endswith("_ms") else box[0][k]) for k in box[0]}
        with open(out, "w") as f:
            json.dump(worst, f)
    router.close()
    dist.destroy_process_group()


def router_case(n, replan):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"migrate_probe_{os.getpid()}.json")
    mp.spawn(_rank, args=(port, n, replan, out), nprocs=WORLD, join=True)
    res = json.load(open(out))
    os.remove(out)
    res.update(batch_per_rank=n, transport="host", lib=rl_amd.LIB_PATH)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["engine", "replan"], choices=["engine", "replan", "step"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--population", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=1 << 20, help="requests per rank per router step")
    a = ap.parse_args()
    res = {"reps": a.reps}
    # the two-rank parts first: their workers are started before this process opens the GPU
    if "replan" in a.parts:
        res["replan"] = router_case(a.batch, True)
    if "step" in a.parts:
        res["step"] = router_case(a.batch, False)
    if "engine" in a.parts:
        res["engine"] = [c for n_lim in (1, 2, 10) for c in engine_case(n_lim, a.population, a.reps)]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
