#!/usr/bin/env python3
"""Time of rl_quota_device beside the calls it replaces, on the same queries in one run:
rl_retry_after_device (the Retry-After number) and one rl_execute_batch_device batch of RL_OP_PEEK
over the same keys (the X-RateLimit-Remaining number; nothing but rl_quota computes the reset).

Table: bench.py's tb_uniform (TB 50 @ 10/s, window 60 s, 1M keys) after one 16M-request batch.
Queries: 2^20 uniform keys of the same population, permits 1-3, at the trace end. Every call takes
the same caller stream and is bracketed by events on it; warm, median of 10. The claim to check:
the fused call costs less than the retry call plus the peek batch. The answers are cross-checked:
remaining against the PEEK batch, retry_ms against rl_retry_after_device.

usage: tools/quota_probe.py [--queries 1048576] [--batch 16777216] [--keys 1000000] [--reps 10]
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
T0_NS = 1_700_000_000_000 * NS
SPAN_NS = 2_000 * NS
SEED = 0x5EED0002


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
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=1 << 24)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = "cuda"
    e = rl_amd.Engine(max_batch=max(a.batch, a.queries), capacity=a.keys)
    e.add_limiter(rl_amd.TB, 50, 60_000, 10.0)

    def arrays(n):
        return (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                torch.empty(n, dtype=torch.int64, device=dev))

    # ---- the table: one tb_uniform batch
    k, p, t = arrays(a.batch)
    al = torch.empty(a.batch, dtype=torch.uint8, device=dev)
    rem = torch.empty(a.batch, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    e.synth_trace(a.batch, k, p, t, None, seed=SEED, n_keys=a.keys, permits_max=4, t0_ns=T0_NS,
                  span_ns=SPAN_NS)
    e.execute_device(a.batch, k, p, t, None, None, al, rem)
    st = e.last_status()
    assert st == rl_amd.RL_OK, rl_amd.strerror(st)
    denied = 1.0 - float(al.sum().item()) / a.batch
    del k, p, t, al, rem

    # ---- the queries: other draws of the same key population, all at the trace end
    n = a.queries
    qk, qp, qt = arrays(n)
    e.synth_trace(n, qk, qp, qt, None, seed=SEED, n_keys=a.keys, permits_max=3,
                  t0_ns=T0_NS + SPAN_NS, span_ns=0, index_base=a.batch, n_total=n)
    e.sync()
    peek = torch.full((n,), rl_amd.OP_PEEK, dtype=torch.uint8, device=dev)
    pa = torch.empty(n, dtype=torch.uint8, device=dev)
    pr = torch.empty(n, dtype=torch.int64, device=dev)
    wait = torch.empty(n, dtype=torch.int64, device=dev)
    q3 = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3)]
    q2 = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = s.cuda_stream

    peek_ms = timed(s, a.reps, lambda: e.execute_device(n, qk, qp, qt, None, peek, pa, pr, stream=sp))
    assert e.last_status() == rl_amd.RL_OK
    retry_ms = timed(s, a.reps, lambda: e.retry_after_device(n, qk, qp, qt, None, None, wait, stream=sp))
    quota_ms = timed(s, a.reps, lambda: e.quota_device(n, qk, qt, None, qp, None, *q3, stream=sp))
    plain_ms = timed(s, a.reps, lambda: e.quota_device(n, qk, qt, None, None, None, q2[0], q2[1], None,
                                                       stream=sp))
    torch.cuda.synchronize()

    # the calls agree with each other
    rem3, rst3, rty3 = (x.cpu().numpy() for x in q3)
    rem2, rst2 = (x.cpu().numpy() for x in q2)
    assert np.array_equal(rem3, pr.cpu().numpy()), "remaining must be the PEEK batch's"
    assert np.array_equal(rty3, wait.cpu().numpy()), "retry_ms must be rl_retry_after_device's"
    assert np.array_equal(rem2, rem3) and np.array_equal(rst2, rst3)
    assert np.array_equal(rst3 == 0, rem3 == 50) and rst3.min() >= 0

    def leg(ms):
        return {"ms": round(ms, 4), "queries_per_s": round(n / ms * 1e3)}

    out = {
        "table": f"tb_uniform: TB 50 @ 10/s, {a.keys} keys, after one {a.batch}-request batch "
                 f"({denied:.3f} of it denied)",
        "queries": n, "reset_positive_share": round(float((rst3 > 0).mean()), 4),
        "retry_positive_share": round(float((rty3 > 0).mean()), 4),
        "max_reset_ms": int(rst3.max()),
        "device": torch.cuda.get_device_name(0),
        "peek_batch": leg(peek_ms),
        "retry_after": leg(retry_ms),
        "quota_with_permits": leg(quota_ms),
        "quota_without_permits": leg(plain_ms),
        "retry_plus_peek_over_quota": round((retry_ms + peek_ms) / quota_ms, 2),
        "fused_is_cheaper": bool(quota_ms < retry_ms + peek_ms),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
