#!/usr/bin/env python3
"""Time of rl_shrink_plan and rl_shrink_limiter on a large table that is mostly expired, beside
rl_sweep_expired on the same table: the sweep is the yardstick, it reads the same bytes and
writes more (every region back in place; the shrink's first pass writes 1/8 of them).

The table: one token bucket limiter (window 60 s, so a bucket lives 120 s) sized for `--keys`
keys; a flood of one batch of `--flood` uniform requests over that many keys at t0; 130 s later
`--regulars` keys come once. Everything of the flood is dead by then. At t0 + 131 s the plan is
timed (it only reads: one warm-up call, then the median of `--reps`), then the sweep on one engine
and the shrink on a second engine with the same contents (both change the table, so each is one
call per engine pair; `--pairs` pairs, the median over them). A small engine runs all three
first so that no call pays for loading its kernels. Each call synchronises itself and is timed
on the host clock around the call.

The peak extra device memory of the shrink is computed from what the call allocates: the merge
passes' tables (rl_shrink.hpp: 3 halvings per pass, the remainder last) and 12 B per region of
plan scratch + the control block.

usage: tools/shrink_probe.py [--keys 8000000] [--flood 16777216] [--regulars 65536] [--reps 7] [--pairs 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rl_amd  # noqa: E402

NS = 1_000_000
T0_NS = 1_700_000_000_000 * NS
LIMITER = (rl_amd.TB, 50, 60_000, 10.0)
HBM_BYTES_PER_S = 8e12


def ms_of(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def filled(keys, flood, regulars, max_batch):
    """An engine after the flood and the regulars; returns (engine, now_ns of the probe)."""
    e = rl_amd.Engine(max_batch=max_batch, capacity=keys)
    e.add_limiter(*LIMITER)
    allowed = torch.empty(max_batch, dtype=torch.uint8, device="cuda")
    remaining = torch.empty(max_batch, dtype=torch.int64, device="cuda")
    for n, n_keys, t0, seed in ((flood, keys, T0_NS, 0x5EED0F10), (regulars, regulars, T0_NS + 130_000 * NS, 0x5EED0F11)):
        k = torch.empty(n, dtype=torch.int64, device="cuda")
        p = torch.empty(n, dtype=torch.int32, device="cuda")
        t = torch.empty(n, dtype=torch.int64, device="cuda")
        lim = torch.empty(n, dtype=torch.int16, device="cuda")
        e.synth_trace(n, k, p, t, lim, seed=seed, n_keys=n_keys, permits_max=2, t0_ns=t0, span_ns=500 * NS)
        e.sync()
        e.execute_device(n, k, p, t, lim, None, allowed, remaining)
        st = e.last_status()
        assert st == rl_amd.RL_OK, rl_amd.strerror(st)
        del k, p, t, lim
    return e, T0_NS + 131_000 * NS


def extra_bytes(report, cache=False):
    """Device memory rl_shrink_limiter allocates for this plan, all of it live at the last pass."""
    per_slot = 32 + (8 if cache else 0)
    regions = report["slots_before"] // rl_amd.REGION_SLOTS
    total, slots, j = 120 + 12 * regions + 4, report["slots_before"], report["halvings"]
    while j > 0:
        s = min(3, j)
        slots >>= s
        j -= s
        total += slots * per_slot
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=8_000_000)
    ap.add_argument("--flood", type=int, default=1 << 24)
    ap.add_argument("--regulars", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    max_batch = max(a.flood, a.regulars)

    # warm-up: every kernel of the three calls once, on a small table
    w, now = filled(1 << 16, 1 << 17, 1 << 10, 1 << 17)
    w.shrink_plan(0, now)
    w.sweep_expired(now)
    w.grow_limiter(0, 1 << 18)
    w.shrink_limiter(0, now)
    w.close()

    res = {"device": torch.cuda.get_device_name(0), "keys": a.keys, "flood": a.flood,
           "regulars": a.regulars, "reps": a.reps, "pairs": a.pairs}
    plan_ms, sweep_ms, shrink_ms = [], [], []
    for pair in range(a.pairs):
        A, now = filled(a.keys, a.flood, a.regulars, max_batch)
        B, _ = filled(a.keys, a.flood, a.regulars, max_batch)
        assert A.limiter_slots(0) == B.limiter_slots(0)
        plan = A.shrink_plan(0, now)
        ms = [ms_of(lambda: A.shrink_plan(0, now))[0] for _ in range(a.reps)]
        plan_ms.append(statistics.median(ms))
        t_sweep, reclaimed = ms_of(lambda: B.sweep_expired(now))
        t_shrink, report = ms_of(lambda: A.shrink_limiter(0, now))
        assert report == plan and reclaimed == plan["used_before"] - plan["kept"]
        assert A.limiter_slots(0) == plan["slots_after"]
        ua, ub = A.limiter_usage(0, now), B.limiter_usage(0, now)
        assert ua["used_slots"] == ub["used_slots"] == ua["live_keys"] == ub["live_keys"] == plan["kept"]
        assert ua["used_permits"] == ub["used_permits"]
        sweep_ms.append(t_sweep)
        shrink_ms.append(t_shrink)
        if pair == 0:
            table_bytes = plan["slots_before"] * 32
            res.update(plan={k: v for k, v in plan.items()}, table_bytes=table_bytes,
                       shrink_passes=(plan["halvings"] + 2) // 3,
                       shrink_extra_bytes=extra_bytes(plan),
                       shrink_extra_share_of_table=round(extra_bytes(plan) / table_bytes, 4))
        A.close()
        B.close()
        torch.cuda.empty_cache()
    med = lambda v: round(statistics.median(v), 4)  # noqa: E731
    res.update(plan_ms=[med(plan_ms), round(min(plan_ms), 4), round(max(plan_ms), 4)],
               sweep_ms=[med(sweep_ms), round(min(sweep_ms), 4), round(max(sweep_ms), 4)],
               shrink_ms=[med(shrink_ms), round(min(shrink_ms), 4), round(max(shrink_ms), 4)])
    res["plan_bytes_per_s"] = round(res["table_bytes"] / (res["plan_ms"][0] * 1e-3))
    res["plan_share_of_8TBps"] = round(res["plan_bytes_per_s"] / HBM_BYTES_PER_S, 4)
    res["shrink_over_sweep"] = round(res["shrink_ms"][0] / res["sweep_ms"][0], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
