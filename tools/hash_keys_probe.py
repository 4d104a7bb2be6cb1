#!/usr/bin/env python3
"""Time of rl_hash_keys_device on 2^24 keys in device memory at three shapes (lengths uniform in
8..40, all keys 16 bytes, lengths uniform in 200..400), in one process and alternating per
repetition:
  tile     the kernel as shipped (LDS-staged spans, direct reads where a span exceeds the tile)
  direct   the same kernel with rl_tune("keys_direct", 1): one lane per key reading its bytes
           from global memory, the plain baseline
  copy     a device-to-device copy of the same byte count (torch), what bytes/s is read against
Each is timed with device events on one stream after a warm-up: the median of `--reps`
repetitions, min and max beside it. The kernel's bytes are blob + 8 (n + 1) + 8 n. Both kernel
paths are checked against rl_key_hash on the host over every key, and that host pass is timed on
`--threads` host threads (tools/hash_keys_host.cpp): the work this feature takes off a front-end.

usage: tools/hash_keys_probe.py [--log2-keys 24] [--reps 20] [--threads 16] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rl_amd  # noqa: E402

SHAPES = [("uniform_8_40", 8, 40), ("all_16", 16, 16), ("uniform_200_400", 200, 400)]
HOST_LIB = os.path.join(rl_amd.PKG_DIR, "bin", "libhash_keys_host.so")


def host_lib():
    src = os.path.join(ROOT, "tools", "hash_keys_host.cpp")
    if not os.path.exists(HOST_LIB) or os.path.getmtime(HOST_LIB) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(HOST_LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", HOST_LIB, src,
                               "-L" + rl_amd.PKG_DIR, "-lrl_engine", "-Wl,-rpath," + rl_amd.PKG_DIR,
                               "-pthread"])
    rl_amd.lib()                                     # (librl_engine.so first: one HIP runtime)
    h = ctypes.CDLL(HOST_LIB)
    h.hash_keys_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                 ctypes.c_void_p]
    h.hash_keys_host.restype = None
    return h


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4)}


def probe(e, name, lo, hi, n, reps, threads, host):
    # a stream of torch's own (not the null stream), so that the engine joins it and the events
    # on it bracket the kernel
    with torch.cuda.stream(torch.cuda.Stream()):
        return probe_on_stream(e, name, lo, hi, n, reps, threads, host)


def probe_on_stream(e, name, lo, hi, n, reps, threads, host):
    g = torch.Generator(device="cuda").manual_seed(lo * 1000 + hi)
    lens = torch.randint(lo, hi + 1, (n,), generator=g, device="cuda", dtype=torch.int64)
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens, 0)
    blob_bytes = int(off[-1])
    blob = torch.randint(0, 256, (blob_bytes,), generator=g, device="cuda", dtype=torch.uint8)
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    hdr = torch.zeros(2, dtype=torch.int64, device="cuda")
    moved = blob_bytes + 8 * (n + 1) + 8 * n
    src = torch.empty(moved, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    stream = torch.cuda.current_stream().cuda_stream
    assert stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def kernel(direct):
        e.tune("keys_direct", direct)
        e.hash_keys_device(n, blob, blob_bytes, off, out, hdr, stream=stream)

    runs = {"tile": lambda: kernel(0), "direct": lambda: kernel(1), "copy": lambda: dst.copy_(src)}
    ms = {k: [] for k in runs}
    for rep in range(reps + 2):                      # the first two rounds warm up
        for k, fn in runs.items():
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            if rep >= 2:
                ms[k].append(ev[0].elapsed_time(ev[1]))
    e.tune("keys_direct", 0)

    # every key of both paths against rl_key_hash on the host, which is timed
    h_blob, h_off = blob.cpu().numpy(), off.cpu().numpy().view(np.uint64)
    want = np.zeros(n, np.uint64)
    host_ms = []
    for _ in range(3):
        t = time.perf_counter()
        host.hash_keys_host(h_blob.ctypes.data, h_off.ctypes.data, n, threads, want.ctypes.data)
        host_ms.append((time.perf_counter() - t) * 1e3)
    assert int(want[0]) == rl_amd.key_hash(h_blob[:int(h_off[1])].tobytes())
    for direct in (0, 1):
        out.zero_()
        kernel(direct)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want), (name, direct)
        assert hdr.tolist() == [0, n]
    e.tune("keys_direct", 0)

    res = {"shape": name, "keys": n, "blob_bytes": blob_bytes, "kernel_bytes": moved,
           "tile": stats(ms["tile"]), "direct": stats(ms["direct"]), "copy_same_bytes": stats(ms["copy"]),
           "host_threads": threads, "host": stats(host_ms)}
    for k in ("tile", "direct"):
        res[k]["keys_per_s"] = round(n / (res[k]["median_ms"] * 1e-3))
        res[k]["kernel_bytes_per_s"] = round(moved / (res[k]["median_ms"] * 1e-3))
    res["copy_same_bytes"]["copied_bytes_per_s"] = round(moved / (res["copy_same_bytes"]["median_ms"] * 1e-3))
    res["host"]["keys_per_s"] = round(n / (res["host"]["median_ms"] * 1e-3))
    res["tile_over_direct"] = round(res["tile"]["median_ms"] / res["direct"]["median_ms"], 4)
    res["tile_over_copy"] = round(res["tile"]["median_ms"] / res["copy_same_bytes"]["median_ms"], 4)
    res["host_over_tile"] = round(res["host"]["median_ms"] / res["tile"]["median_ms"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-keys", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--shapes", nargs="+", default=[s[0] for s in SHAPES])
    ap.add_argument("--out", default="", help="also write the result JSON to this file")
    a = ap.parse_args()
    host = host_lib()
    e = rl_amd.Engine(max_batch=1 << 16, capacity=1 << 12)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "timing": "device events, per call",
           "cases": []}
    for name, lo, hi in SHAPES:
        if name in a.shapes:
            res["cases"].append(probe(e, name, lo, hi, 1 << a.log2_keys, a.reps, a.threads, host))
            print(json.dumps(res["cases"][-1]), flush=True)
            torch.cuda.empty_cache()
            if a.out:                                # (after every case: a later one may not fit)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
