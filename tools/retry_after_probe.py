#!/usr/bin/env python3
"""Throughput of rl_retry_after_device on the tb_uniform table, beside the only other way to ask
the table anything: one rl_execute_batch_device batch of RL_OP_PEEK over the same keys.

Table: bench.py's tb_uniform (TB 50 @ 10/s, window 60 s, 1M keys) after one 64M-request batch.
Queries: 2^24 uniform keys of the same population, permits 1-3, at the trace end; once with
skip = NULL and once with skip = allowed, where allowed = (the PEEK batch's balance >= permits),
i.e. what a batch's own `allowed` would hand back. Both calls take the same caller stream and
are bracketed by events on it; warm, median of 10. Bytes per query = 20 B in + 8 B out +
128 B per probed bucket; the probed buckets and the share of searches that fell back to
bisection come from a measurement build's counters (tools/build_variant.sh <name>
"-DRL_RETRY_COUNT", run with RL_ENGINE_LIB=.../variants/<name>/librl_engine.so): the product
build has none, and the counting build's times are not the product's.

usage: tools/retry_after_probe.py [--queries 16777216] [--batch 67108864] [--reps 10]
"""
import argparse
import ctypes
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


def counters(e):
    out = np.zeros(3, np.uint64)
    k = e._L.rl_debug_fetch(e.handle, b"retry_counts", rl_amd._p(out), out.nbytes)
    return None if k < 0 else [int(x) for x in out]


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
    ap.add_argument("--queries", type=int, default=1 << 24)
    ap.add_argument("--batch", type=int, default=1 << 26)
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
    wait2 = torch.empty(n, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = s.cuda_stream

    peek_ms = timed(s, a.reps, lambda: e.execute_device(n, qk, qp, qt, None, peek, pa, pr, stream=sp))
    assert e.last_status() == rl_amd.RL_OK
    allowed = (pr >= qp.to(torch.int64)).to(torch.uint8).contiguous()
    torch.cuda.synchronize()
    counters(e)                                      # (measurement build: start from zero)
    full_ms = timed(s, a.reps, lambda: e.retry_after_device(n, qk, qp, qt, None, None, wait, stream=sp))
    c_full = counters(e)
    skip_ms = timed(s, a.reps, lambda: e.retry_after_device(n, qk, qp, qt, None, allowed, wait2, stream=sp))
    c_skip = counters(e)
    torch.cuda.synchronize()

    # the two query calls agree with each other and with the PEEK batch
    w, w2, alw = wait.cpu().numpy(), wait2.cpu().numpy(), allowed.cpu().numpy() != 0
    assert np.array_equal(w == 0, alw), "wait == 0 must be exactly balance >= permits"
    assert np.array_equal(w2[~alw], w[~alw]) and not w2[alw].any()

    def leg(ms, c, skipped):
        o = {"ms": round(ms, 4), "queries_per_s": round(n / ms * 1e3)}
        if c:                                        # counts of reps + 1 identical runs
            runs = a.reps + 1
            buckets = c[2] / runs
            o["bytes_per_query"] = round(28 + 128 * buckets / n, 2)
            o["buckets_per_lookup"] = round(buckets / max(1, n - skipped), 4)
            o["searches_per_run"] = c[0] // runs
            o["bisection_share_of_searches"] = round(c[1] / max(1, c[0]), 6)
        return o

    out = {
        "table": f"tb_uniform: TB 50 @ 10/s, {a.keys} keys, after one {a.batch}-request batch "
                 f"({denied:.3f} of it denied)",
        "queries": n, "wait_positive_share": round(float((w > 0).mean()), 4),
        "max_wait_ms": int(w.max()),
        "measurement_build": c_full is not None,
        "device": torch.cuda.get_device_name(0),
        "peek_batch": {"ms": round(peek_ms, 4), "queries_per_s": round(n / peek_ms * 1e3)},
        "retry_after": leg(full_ms, c_full, 0),
        "retry_after_skip_allowed": leg(skip_ms, c_skip, int(alw.sum())),
        "peek_over_retry": round(peek_ms / full_ms, 2),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
