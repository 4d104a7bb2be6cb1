#!/usr/bin/env python3
"""Time of rl_limiter_digest (bucket_bits 0, 12 and the table's region bits; with and without
RL_DIGEST_CACHE is the same pass on the bench limiters, which keep no cache table) beside
rl_limiter_usage, which reads the same bytes, and beside a full rl_snapshot_keys loop, the work a
clean digest saves, in one run on one table.

The table is filled as bench.py fills it: `--steps` batches of the config's synthetic trace
(tb_uniform = BASELINE configs[1], 1M keys; sw_zipf = configs[2], 100M keys) through
rl_execute_batch_device. The calls then run at the trace's end time. Each synchronises itself, so
it is timed on the host clock around the call: after one warm-up call, the median of `--reps`
repetitions (min and max beside it). The digest reads slots x 32 B once; that is set against the
8 TB/s HBM peak.

usage: tools/digest_probe.py [--configs tb_uniform sw_zipf] [--steps 2] [--reps 7] [--snapshot-reps 7]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import rl_amd  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timed(reps, fn):
    ms = []
    for i in range(reps + 1):                       # the first run warms up
        t = time.perf_counter()
        fn()
        if i:
            ms.append((time.perf_counter() - t) * 1e3)
    return [round(x, 4) for x in (statistics.median(ms), min(ms), max(ms))]


def probe(name, steps, reps, snapshot_reps, batch, chunk):
    cfg = bench.CONFIGS[name]
    assert len(cfg["limiters"]) == 1
    n = batch or cfg["batch"]
    e = rl_amd.Engine(max_batch=n, capacity=cfg["capacity"])
    e.add_limiter(*cfg["limiters"][0])
    allowed = torch.empty(n, dtype=torch.uint8, device="cuda")
    remaining = torch.empty(n, dtype=torch.int64, device="cuda")
    for s in range(steps):
        (keys, permits, now, lim), = bench.make_inputs(e, cfg, n, 1, 0, steps, "cuda", first=s, count=1)
        e.sync()
        e.execute_device(n, keys, permits, now, lim, None, allowed, remaining)
        st = e.last_status()
        assert st == rl_amd.RL_OK, rl_amd.strerror(st)
        del keys, permits, now, lim
    del allowed, remaining
    now_ns = bench.T0_NS + cfg["span_ns"] * steps
    slots = e.limiter_slots(0)
    k = (slots // rl_amd.REGION_SLOTS).bit_length() - 1
    out = {"config": name, "requests": n * steps, "slots": slots, "region_bits": k,
           "table_bytes": slots * 32}              # (the bench limiters keep no cache table)

    u = {}
    out["census_ms"] = timed(reps, lambda: u.update(e.limiter_usage(0, now_ns)))
    out["redis_keys"], out["used_slots"] = u["redis_keys"], u["used_slots"]

    out["digest_ms"] = {}
    totals = set()
    for bits in sorted({0, min(12, k), k}):
        buf = np.zeros(1 << bits, rl_amd.DIGEST_DTYPE)
        tot = rl_amd.BucketDigest()
        L = rl_amd.lib()

        def digest():
            st = L.rl_limiter_digest(e.handle, 0, now_ns, bits, rl_amd.DIGEST_CACHE, rl_amd._p(buf),
                                     ctypes.byref(tot))
            assert st == rl_amd.RL_OK, rl_amd.strerror(st)

        out["digest_ms"][str(bits)] = timed(reps, digest)
        totals.add((tot.entries, tot.sum, tot.xr))
    assert len(totals) == 1 and next(iter(totals))[0] == u["redis_keys"], (totals, u["redis_keys"])
    out["digest_total"] = [hex(x) for x in next(iter(totals))]
    d0 = out["digest_ms"]["0"][0]
    out["digest_bytes_per_s"] = round(out["table_bytes"] / (d0 * 1e-3))
    out["digest_share_of_8TBps"] = round(out["digest_bytes_per_s"] / HBM_BYTES_PER_S, 4)
    out["digest_over_census"] = {b: round(v[0] / out["census_ms"][0], 2) for b, v in out["digest_ms"].items()}

    images = np.zeros(chunk, rl_amd.KEY_IMAGE_DTYPE)
    count = {}

    def snapshot():
        at, total, got = 0, 1, 0
        while at < total:
            _, st, m, done, total = e.snapshot_keys(0, at, 1 << 62, chunk, out=images)
            assert st == rl_amd.RL_OK and done > 0
            at += done
            got += m
        count["n"] = got

    out["snapshot_ms"] = timed(snapshot_reps, snapshot)
    out["snapshot_images"] = count["n"]
    out["snapshot_bytes"] = count["n"] * rl_amd.KEY_IMAGE_DTYPE.itemsize
    out["digest_over_snapshot"] = {b: round(v[0] / out["snapshot_ms"][0], 5) for b, v in out["digest_ms"].items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["tb_uniform", "sw_zipf"])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--snapshot-reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=0, help="requests per step (default: the config's)")
    ap.add_argument("--chunk", type=int, default=1 << 20, help="images per rl_snapshot_keys call")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "snapshot_reps": a.snapshot_reps,
           "cases": []}
    for name in a.configs:
        res["cases"].append(probe(name, a.steps, a.reps, a.snapshot_reps, a.batch, a.chunk))
        print(json.dumps(res["cases"][-1]), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
