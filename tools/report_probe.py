#!/usr/bin/env python3
"""Time of the batch report on a batch's own outputs: rl_tally_batch_device and
rl_top_denied_device, beside rl_top_keys_device on the same key array (the existing call the
selector passes are derived from, and so their yardstick).

Batch: bench.py's sw_zipf scaled to one quarter (SW 1000 per 60 s, Zipf 1.1 over 25M keys, 2^26
requests over 60 s), executed once; the three calls then read its arrays. All take the same
caller stream and are bracketed by events on it; warm, median of 10. Bytes read per request:
tally 12 (limiter and op are NULL here; 16 with both), top-denied 2 passes x 21 (24 with both),
top-keys 2 passes x 8. The answers are checked against each other: the tally's denied count is
top-denied's |S|, and every key top-denied returns is counted at least as often by top-keys.

usage: tools/report_probe.py [--batch 67108864] [--keys 25000000] [--reps 10]
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
SEED = 0x5EED0003


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
    ap.add_argument("--batch", type=int, default=1 << 26)
    ap.add_argument("--keys", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--min-count", type=int, default=1000)
    a = ap.parse_args()
    dev, n = "cuda", a.batch
    e = rl_amd.Engine(max_batch=n, capacity=a.keys)
    e.add_limiter(rl_amd.SW, 1000, 60_000)
    k = torch.empty(n, dtype=torch.int64, device=dev)
    p = torch.empty(n, dtype=torch.int32, device=dev)
    t = torch.empty(n, dtype=torch.int64, device=dev)
    al = torch.empty(n, dtype=torch.uint8, device=dev)
    rem = torch.empty(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    e.synth_trace(n, k, p, t, None, seed=SEED, n_keys=a.keys, dist=rl_amd.DIST_ZIPF, zipf_s=1.1,
                  permits_max=1, t0_ns=T0_NS, span_ns=60_000 * NS)
    e.execute_device(n, k, p, t, None, None, al, rem)
    st = e.last_status()
    assert st == rl_amd.RL_OK, rl_amd.strerror(st)

    out = torch.zeros(rl_amd.TALLY_ROWS * 12, dtype=torch.int64, device=dev)
    dk = torch.zeros(a.k, dtype=torch.int64, device=dev)
    dc = torch.zeros(a.k, dtype=torch.int64, device=dev)
    dh = torch.zeros(4, dtype=torch.int64, device=dev)
    tk = torch.zeros(a.k, dtype=torch.int64, device=dev)
    tc = torch.zeros(a.k, dtype=torch.int64, device=dev)
    th = torch.zeros(4, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = s.cuda_stream
    L, h, ptr = e._L, e.handle, rl_amd._p

    def top_denied():
        st = L.rl_top_denied_device(h, n, ptr(k), ptr(p), None, None, ptr(al), ptr(rem), 0, a.k, a.min_count,
                                    ptr(dk), ptr(dc), ptr(dh), sp)
        assert st == rl_amd.RL_OK

    def top_keys():
        st = L.rl_top_keys_device(h, n, ptr(k), a.k, a.min_count, ptr(tk), ptr(tc), ptr(th), sp)
        assert st == rl_amd.RL_OK

    tally_ms = timed(s, a.reps, lambda: e.tally_batch_device(n, p, None, None, al, rem, out, stream=sp))
    denied_ms = timed(s, a.reps, top_denied)
    keys_ms = timed(s, a.reps, top_keys)
    torch.cuda.synchronize()

    row = out.cpu().numpy().view(rl_amd.TALLY_DTYPE)[0]
    dhdr, thdr = dh.cpu().tolist(), th.cpu().tolist()
    assert int(row["requests"]) == n and int(row["allowed"]) == int(al.sum().item())
    assert dhdr[2] == 0 and thdr[2] == 0 and dhdr[3] == int(row["denied"])
    all_counts = dict(zip(tk.cpu().numpy().view(np.uint64)[:thdr[0]].tolist(), tc.cpu().tolist()))
    for key, c in zip(dk.cpu().numpy().view(np.uint64)[:dhdr[0]].tolist(), dc.cpu().tolist()):
        assert key not in all_counts or all_counts[key] >= c

    def leg(ms, bytes_per_request):
        return {"ms": round(ms, 4), "requests_per_s": round(n / ms * 1e3),
                "bytes_per_s": round(n * bytes_per_request / ms * 1e3)}

    print(json.dumps({
        "batch": f"sw_zipf/4: SW 1000 per 60 s, Zipf 1.1 over {a.keys} keys, {n} requests",
        "denied_share": round(int(row["denied"]) / n, 4),
        "k": a.k, "min_count": a.min_count, "device": torch.cuda.get_device_name(0),
        "tally": leg(tally_ms, 12),
        "top_denied": dict(leg(denied_ms, 42), n_out=dhdr[0], n_heavy=dhdr[1]),
        "top_keys": dict(leg(keys_ms, 16), n_out=thdr[0], n_heavy=thdr[1]),
        "top_denied_over_top_keys": round(denied_ms / keys_ms, 2),
    }))


if __name__ == "__main__":
    main()
