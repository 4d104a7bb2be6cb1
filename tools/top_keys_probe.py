#!/usr/bin/env python3
"""Time of rl_top_keys_device beside the only other producer of the router's directory
candidates: bench.plan_directory's torch.unique(return_counts=True) + torch.topk on the same
device keys.

Inputs: the first 2^22 keys of bench.py's sw_zipf trace (100M keys, Zipf s = 1.1) with
k = 4096, min_count = 50, and the first 2^26 keys of the same trace (min_count 50 and 800).
Both paths run on one torch stream, bracketed by events on it; after a warm-up run, the median
of 20 repetitions. The new call streams the keys twice: 2 x 8 B x n, set against the 6.3 TB/s
copy rate. The torch path's counts are compared with the call's (its order among equal counts
is not the contract's, so keys are compared as sets above the cut).

usage: tools/top_keys_probe.py [--reps 20] [--sizes 22 26]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rl_amd  # noqa: E402

NS = 1_000_000
COPY_BYTES_PER_S = 6.3e12
SW_ZIPF = dict(seed=0x5EED0003, n_keys=100_000_000, dist=rl_amd.DIST_ZIPF, zipf_s=1.1, permits_max=1,
               span_ns=60_000 * NS, n_total=1 << 28)


def timed(stream, reps, fn):
    ms = []
    for i in range(reps + 1):                       # the first run warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        stream.synchronize()
        if i:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[22, 26], help="log2 of the sample sizes")
    ap.add_argument("--k", type=int, default=4096)
    a = ap.parse_args()
    dev = "cuda"
    n_max = 1 << max(a.sizes)
    e = rl_amd.Engine(max_batch=n_max, capacity=1 << 12)
    keys = torch.empty(n_max, dtype=torch.int64, device=dev)
    permits = torch.empty(n_max, dtype=torch.int32, device=dev)
    now = torch.empty(n_max, dtype=torch.int64, device=dev)
    e.synth_trace(n_max, keys, permits, now, None, **SW_ZIPF)
    e.sync()
    del permits, now
    s = torch.cuda.Stream()
    top = torch.empty(a.k, dtype=torch.int64, device=dev)
    cnt = torch.empty(a.k, dtype=torch.int64, device=dev)
    hdr = torch.empty(4, dtype=torch.int64, device=dev)
    L = rl_amd.lib()
    out = {"device": torch.cuda.get_device_name(0), "k": a.k, "reps": a.reps, "cases": []}
    for lg in a.sizes:
        n = 1 << lg
        sample = keys[:n]
        for min_count in ((50,) if lg <= 22 else (50, 800)):
            def ours():
                st = L.rl_top_keys_device(e.handle, n, rl_amd._p(sample), a.k, min_count, rl_amd._p(top),
                                          rl_amd._p(cnt), rl_amd._p(hdr), s.cuda_stream)
                assert st == rl_amd.RL_OK, rl_amd.strerror(st)

            res = {}

            def theirs():
                with torch.cuda.stream(s):
                    u, c = torch.unique(sample, return_counts=True)
                    t = torch.topk(c, min(a.k, c.numel()))
                    res["u"], res["c"], res["t"] = u, c, t

            torch.cuda.synchronize()
            ours_ms = timed(s, a.reps, ours)
            h = [int(x) for x in hdr.cpu()]
            case = {"n": n, "min_count": min_count, "hdr": h,
                    "top_keys_ms": [round(x, 4) for x in ours_ms],
                    "bytes_streamed": 16 * n,
                    "stream_floor_ms": round(16 * n / COPY_BYTES_PER_S * 1e3, 4)}
            case["floor_share"] = round(case["stream_floor_ms"] / ours_ms[0], 3)
            if min_count == 50:
                torch_ms = timed(s, a.reps, theirs)
                case["torch_unique_topk_ms"] = [round(x, 4) for x in torch_ms]
                case["torch_over_top_keys"] = round(torch_ms[0] / ours_ms[0], 2)
                case["distinct"] = int(res["c"].numel())
                if not h[2]:                         # same counts; same keys above the cut's count
                    tc = res["t"].values.cpu().numpy()
                    tk = res["u"][res["t"].indices].cpu().numpy().view(np.uint64)
                    m = tc >= min_count
                    gc = cnt[:h[0]].cpu().numpy().view(np.uint64).astype(np.int64)
                    gk = top[:h[0]].cpu().numpy().view(np.uint64)
                    assert h[0] == int(m.sum()) and np.array_equal(gc, tc[m]), "counts differ"
                    above = gc > gc[-1] if h[0] else gc > 0
                    assert set(gk[above].tolist()) == set(tk[m][above].tolist()), "keys differ"
                    assert h[1] == int((res["c"] >= min_count).sum().item()), "n_heavy differs"
                    case["checked_against_torch"] = True
            out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
