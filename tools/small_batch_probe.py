#!/usr/bin/env python3
"""Host-call latency of small batches: the wall time of rl_try_acquire_batch (host buffers, the
call returns the decisions) and of rl_execute_batch_device followed by rl_last_status (device
buffers, the status read waits for the batch), p50 and p99 over `--calls` calls after `--warmup`
warm-up calls, at n = 1, 8, 64, 256, 1024 and RL_SMALL_BATCH_MAX.

One sliding-window and one token-bucket limiter, keys uniform over 1M, every call's timestamps
2 ms after the previous call's. A variant is a library and a value of rl_tune("small_batch"):
  name=path/to/librl_engine.so[:small_batch]
(a library without the key, such as the parent commit's built by tools/build_variant.sh, is
given without a value). Each variant runs in a process of its own (one library per process);
the variants are run one after the other, and the whole set `--repeat` times, so that the
spread between two runs of the same variant is seen beside the difference between variants.
Prints one JSON line per (repeat, variant) and a table of p50 / p99 in microseconds at the end.

usage: tools/small_batch_probe.py parent=variants/parent/librl_engine.so off=librl_engine.so:0 \\
           on=librl_engine.so:1024 [--calls 2000] [--warmup 200] [--repeat 2]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY = os.path.join(ROOT, "distributed-rate-limiter_amd", "python")
SMALL_MAX = 1024                                   # RL_SMALL_BATCH_MAX
SIZES = sorted({1, 8, 64, 256, 1024, SMALL_MAX})
T0_NS = 1_700_000_000_000 * 1_000_000


def percentiles(us):
    import numpy as np
    a = np.sort(np.asarray(us))
    return round(float(a[len(a) // 2]), 2), round(float(a[min(len(a) - 1, (len(a) * 99) // 100)]), 2)


def child(lib_path, small, calls, warmup):
    sys.path[:0] = [ROOT, PY]
    import numpy as np
    import torch
    import rl_amd
    rl_amd.LIB_PATH = os.path.abspath(lib_path)
    e = rl_amd.Engine(max_batch=1 << 16, capacity=1 << 21)
    e.add_limiter(rl_amd.SW, 100, 1000, 0.0)
    e.add_limiter(rl_amd.TB, 100, 1000, 50.0)
    if small is not None:
        e.tune("small_batch", small)
    L, h = e._L, e._h
    rng = np.random.default_rng(1)
    out = {"lib": lib_path, "small_batch": small, "host": {}, "device": {}}
    t_ns = T0_NS
    for n in SIZES:
        total = calls + warmup
        keys = rng.integers(1, 1_000_001, size=(total, n), dtype=np.uint64)
        lim = rng.integers(0, 2, size=(total, n), dtype=np.uint16)
        permits = np.ones(n, np.int32)
        allowed = np.zeros(n, np.uint8)
        remaining = np.zeros(n, np.int64)
        p = rl_amd._p
        us = []
        for c in range(total):
            now = np.full(n, t_ns, np.int64)
            t_ns += 2_000_000
            k, l = keys[c], lim[c]
            t = time.perf_counter()
            st = L.rl_try_acquire_batch(h, n, p(k), p(permits), p(now), p(l), p(allowed), p(remaining), None)
            dt = time.perf_counter() - t
            assert st == rl_amd.RL_OK, rl_amd.strerror(st)
            if c >= warmup:
                us.append(dt * 1e6)
        out["host"][n] = percentiles(us)
        # device buffers: the inputs are staged before the clock starts
        dk = torch.from_numpy(keys.view(np.int64)).cuda()
        dl = torch.from_numpy(lim.view(np.int16)).cuda()
        dp = torch.from_numpy(permits).cuda()
        da = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dr = torch.zeros(n, dtype=torch.int64, device="cuda")
        dnow = torch.full((total, n), 0, dtype=torch.int64, device="cuda")
        dnow += (t_ns + 2_000_000 * torch.arange(total, device="cuda", dtype=torch.int64))[:, None]
        t_ns += 2_000_000 * total
        torch.cuda.synchronize()
        us = []
        for c in range(total):
            t = time.perf_counter()
            e.execute_device(n, dk[c].data_ptr(), dp.data_ptr(), dnow[c].data_ptr(), dl[c].data_ptr(), None,
                             da.data_ptr(), dr.data_ptr())
            st = L.rl_last_status(h)
            dt = time.perf_counter() - t
            assert st == rl_amd.RL_OK, rl_amd.strerror(st)
            if c >= warmup:
                us.append(dt * 1e6)
        out["device"][n] = percentiles(us)
    if small is not None:
        out["taken"], out["declined"] = e.small_batches()
    e.close()
    print("PROBE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("variants", nargs="+", help="name=library[:small_batch]")
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        lib_path, small = a.child
        child(lib_path, None if small == "-" else int(small), a.calls, a.warmup)
        return
    rows = []
    for rep in range(a.repeat):
        for v in a.variants:
            name, spec = v.split("=", 1)
            lib_path, _, small = spec.partition(":")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "x=x", "--calls", str(a.calls), "--warmup",
                                str(a.warmup), "--child", lib_path, small or "-"], capture_output=True, text=True,
                               timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")]
            if r.returncode != 0 or not line:
                sys.exit(f"variant {name} failed (exit {r.returncode}):\n{r.stdout}\n{r.stderr}")
            res = json.loads(line[0][6:])
            res.update(variant=name, repeat=rep)
            print(json.dumps(res), flush=True)
            rows.append(res)
    for form in ("host", "device"):
        print(f"\n{form} form, p50 / p99 in us")
        print("n".rjust(6) + "".join(f"{r['variant']}#{r['repeat']}".rjust(20) for r in rows))
        for n in SIZES:
            print(str(n).rjust(6) + "".join(f"{r[form][str(n)][0]:9.1f} /{r[form][str(n)][1]:8.1f}" for r in rows))


if __name__ == "__main__":
    main()
