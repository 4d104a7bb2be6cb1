#!/usr/bin/env python3
"""Time of rl_limiter_usage and rl_top_consumers(k = 4096, min_used = 1) beside the existing way
to look into a limiter's table, rl_export_state, in one run on one table.

The table is filled as bench.py fills it: `--steps` batches of the config's synthetic trace
(tb_uniform = BASELINE configs[1], 1M keys; sw_zipf = configs[2], 100M keys) through
rl_execute_batch_device. The three calls then run at the trace's end time. Each synchronises
itself, so it is timed on the host clock around the call: after one warm-up call, the median of
`--reps` repetitions (min and max beside it). The census reads slots x 32 B (+ 8 B per slot with
a cache table) once; that is set against the 8 TB/s HBM peak.

usage: tools/usage_probe.py [--configs tb_uniform sw_zipf] [--steps 2] [--reps 7] [--export-reps 5]
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


def probe(name, steps, reps, export_reps, batch):
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
    L = rl_amd.lib()
    out = {"config": name, "requests": n * steps, "grows": e.stats()["table_grows"]}

    u = {}
    out["census_ms"] = timed(reps, lambda: u.update(e.limiter_usage(0, now_ns)))
    out["usage"] = u
    table_bytes = u["slots"] * 32                    # (the bench limiters keep no cache table)
    out["census_bytes"] = table_bytes
    out["census_bytes_per_s"] = round(table_bytes / (out["census_ms"][0] * 1e-3))
    out["census_share_of_8TBps"] = round(out["census_bytes_per_s"] / HBM_BYTES_PER_S, 4)

    top = {}
    out["top_consumers_ms"] = timed(reps, lambda: top.update(r=e.top_consumers(0, now_ns, 4096, 1)))
    passes = ctypes.c_uint32(0)
    assert L.rl_debug_fetch(e.handle, b"usage_passes", ctypes.byref(passes), 4) == 1
    out["top_consumers_passes"] = passes.value       # digit passes + the compaction
    out["n_match"] = top["r"][2]
    out["top_used_first_last"] = [int(top["r"][1][0]), int(top["r"][1][-1])] if len(top["r"][1]) else []

    cnt = ctypes.c_size_t(0)
    st = L.rl_export_state(e.handle, now_ns, None, 0, ctypes.byref(cnt))
    assert st in (rl_amd.RL_OK, rl_amd.RL_E_TOO_LARGE)
    buf = np.zeros(cnt.value + 1, rl_amd.STATE_DTYPE)

    def export():
        assert L.rl_export_state(e.handle, now_ns, rl_amd._p(buf), buf.shape[0], ctypes.byref(cnt)) == rl_amd.RL_OK

    out["export_state_ms"] = timed(export_reps, export)
    out["export_entries"] = cnt.value
    out["export_bytes"] = cnt.value * rl_amd.STATE_DTYPE.itemsize
    assert cnt.value == u["redis_keys"], (cnt.value, u["redis_keys"])
    out["export_over_census"] = round(out["export_state_ms"][0] / out["census_ms"][0], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["tb_uniform", "sw_zipf"])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--export-reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0, help="requests per step (default: the config's)")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "export_reps": a.export_reps,
           "cases": []}
    for name in a.configs:
        res["cases"].append(probe(name, a.steps, a.reps, a.export_reps, a.batch))
        print(json.dumps(res["cases"][-1]), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
