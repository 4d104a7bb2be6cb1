#!/usr/bin/env python3
"""Device-event time of the routing kernels behind rl_router_execute / rl_router_retry_after on
one GPU, each as bytes/s over the bytes its arrays hold and as a share of 8 TB/s:

  * rl_route_partition_skip_device at skip shares 0, 0.5 and 0.9 (8 shards), alternated with
    its baseline rl_route_partition_device at the same n. Bytes: every key (8 B) and skip byte
    read twice (count, then scatter) and 4 B of perm per live request;
  * rl_route_fold_ops (4 B perm + 2 B limiter + 1 B op read, 2 B written) and
    rl_route_unfold_ops (2 B read, 2 B + 1 B written), alternated with each other;
  * rl_route_unpack_wait at skip share 0.5 (1 B skip per query; 4 B perm + 8 B read and 8 B
    written per live query; 8 B written per skipped one).

Every call is warmed up, repeated `--reps` times and alternated with its partner in the same
run; the figure is the median, and `spread` is (max - min) / median over the repeats: a
difference inside it is not one. End-to-end multi-GPU query time is not measured here.

usage: tools/router_query_probe.py [--n 16777216 67108864] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import torch  # noqa: E402

import rl_amd  # noqa: E402

PEAK = 8e12
SHARDS = 8


def alternate(stream, reps, fns):
    """Median ms and spread of each fn, run in turn `reps` times after one warm-up round."""
    ms = [[] for _ in fns]
    for i in range(reps + 1):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            stream.synchronize()
            if i:
                ms[j].append(a.elapsed_time(b))
    return [(statistics.median(m), (max(m) - min(m)) / statistics.median(m)) for m in ms]


def leg(ms, spread, nbytes):
    rate = nbytes / (ms * 1e-3)
    return {"ms": round(ms, 4), "spread": round(spread, 3), "bytes": int(nbytes),
            "bytes_per_s": round(rate), "share_of_8TBs": round(rate / PEAK, 4)}


def probe(e, n, reps):
    dev = "cuda"
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    permits = torch.empty(n, dtype=torch.int32, device=dev)
    now = torch.empty(n, dtype=torch.int64, device=dev)
    e.synth_trace(n, keys, permits, now, None, seed=7, n_keys=1_000_000, n_total=n)
    e.sync()
    del permits, now
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    perm0 = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.zeros(SHARDS, dtype=torch.int64, device=dev)
    u = torch.rand(n, device=dev)
    out = {"n": n}
    for share in (0.0, 0.5, 0.9):
        skip = (u < share).to(torch.uint8).contiguous()
        live = n - int(skip.sum().item())
        torch.cuda.synchronize()
        (sk, sk_sp), (base, base_sp) = alternate(s, reps, [
            lambda: e.route_partition_skip_device(n, keys, skip, perm, SHARDS, counts, 1, stream=sp),
            lambda: e.route_partition_device(n, keys, perm0, SHARDS, counts, 1, stream=sp)])
        o = {"skip": leg(sk, sk_sp, 2 * 9 * n + 4 * live),
             "plain_partition": leg(base, base_sp, 2 * 8 * n + 4 * n),
             "skip_over_plain": round(sk / base, 3)}
        if share == 0.0:
            assert torch.equal(perm, perm0)
        out[f"partition_skip_{share}"] = o
        del skip
    # the ops column
    e.route_partition_device(n, keys, perm, SHARDS, counts, 1, stream=sp)
    lim = (torch.arange(n, device=dev) % 3).to(torch.int16)
    op = (torch.arange(n, device=dev) % 3).to(torch.uint8)
    col = torch.empty(n, dtype=torch.int16, device=dev)
    lim_o = torch.empty(n, dtype=torch.int16, device=dev)
    op_o = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    (fo, fo_sp), (un, un_sp) = alternate(s, reps, [
        lambda: e.route_fold_ops(n, perm, lim, op, col, stream=sp),
        lambda: e.route_unfold_ops(n, col, lim_o, op_o, stream=sp)])
    out["fold_ops"] = leg(fo, fo_sp, 9 * n)
    out["unfold_ops"] = leg(un, un_sp, 5 * n)
    del lim, op, col, lim_o, op_o
    # the wait unpack at skip share 0.5, beside a plain partition as the run's yardstick
    skip = (u < 0.5).to(torch.uint8).contiguous()
    live = n - int(skip.sum().item())
    e.route_partition_skip_device(n, keys, skip, perm, SHARDS, counts, 1, stream=sp)
    back = torch.arange(n, dtype=torch.int64, device=dev)
    wait = torch.empty(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    (uw, uw_sp), (base, base_sp) = alternate(s, reps, [
        lambda: e.route_unpack_wait(n, live, perm, back, skip, wait, stream=sp),
        lambda: e.route_partition_device(n, keys, perm0, SHARDS, counts, 1, stream=sp)])
    out["unpack_wait_0.5"] = leg(uw, uw_sp, n + 20 * live + 8 * (n - live))
    out["unpack_wait_0.5"]["plain_partition_ms"] = round(base, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 24, 1 << 26])
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    e = rl_amd.Engine(max_batch=max(a.n), capacity=1 << 10, shard_index=0, shard_count=SHARDS)
    e.add_limiter(rl_amd.TB, 50, 60_000, 10.0)
    res = {"device": torch.cuda.get_device_name(0), "shards": SHARDS, "reps": a.reps,
           "runs": [probe(e, n, a.reps) for n in a.n]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
