#!/usr/bin/env python3
"""Time of a whole-table snapshot and restore, beside what moved a table before them.

For a limiter of each algorithm (token bucket, sliding window, sliding window with the local
cache) holding `--keys` keys in a table sized for them:

new   rl_snapshot_keys_device over the whole table (one call per 65536 regions) and
      rl_put_keys_device of its output into an equal, empty table (the first put inserts, the
      repeats replace: the same region rebuilds), timed with events on the stream the calls are
      given; a device-to-device copy of the same table bytes (slots, + cache words) on that stream
      for scale; and the host forms rl_snapshot_keys / rl_restore_keys with `--chunk` images per
      chunk (max_batch = `--chunk`), timed on the host clock.
ref   rl_export_state of the same table and rl_put_keys of the same images (saved by `new`),
      host clock, into preallocated buffers. This part runs in a child process; with
      `--parent-lib` (and `--parent-pkg`, the directory of that build's rl_amd package) the child
      loads that build of librl_engine.so (RL_ENGINE_LIB), in the same run.

Every figure: after one warm-up, the median of `--reps` repetitions (min, max), in ms.

usage: tools/snapshot_probe.py [--keys 4194304] [--reps 5] [--parent-lib PATH --parent-pkg DIR]
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
# (the `ref` child of an A/B run binds the parent build with the parent's own package)
sys.path[:0] = [ROOT, os.environ.get("RL_PROBE_PKG") or os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rl_amd  # noqa: E402

NS = 1_000_000
T0 = 1_700_000_000_000
ALGOS = {"tb": dict(algo=rl_amd.TB, max_permits=50, window_ms=60_000, refill_per_s=10.0),
         "sw": dict(algo=rl_amd.SW, max_permits=50, window_ms=60_000),
         "sw_cache": dict(algo=rl_amd.SW, max_permits=50, window_ms=60_000, local_cache_ttl_ms=100)}
SNAP_REGIONS = 65536                       # regions one snapshot call handles


def stats(ms):
    return [round(x, 3) for x in (statistics.median(ms), min(ms), max(ms))]


def engine(cfg, n_keys, max_batch):
    e = rl_amd.Engine(max_batch=max_batch, capacity=n_keys, fixed_capacity=True)
    e.add_limiter(capacity=n_keys, **cfg)
    return e


def fill(e, n_keys, max_batch):
    keys = np.random.default_rng(7).permutation(np.arange(1, n_keys + 1, dtype=np.uint64)) * np.uint64(0x9E3779B1)
    for at in range(0, n_keys, max_batch):
        k = keys[at:at + max_batch]
        st = e.execute(k, np.ones(k.size, np.int32), np.full(k.size, T0 * NS, np.int64), None, None,
                       want_tokens=False)[3]
        assert st == rl_amd.RL_OK, rl_amd.strerror(st)


def timed_stream(reps, stream, fn):
    ms = []
    for i in range(reps + 1):                       # the first run warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if i:
            ms.append(a.elapsed_time(b))
    return stats(ms)


def timed_host(reps, fn):
    ms = []
    for i in range(reps + 1):
        t = time.perf_counter()
        fn()
        if i:
            ms.append((time.perf_counter() - t) * 1e3)
    return stats(ms)


def part_new(name, cfg, n_keys, reps, chunk, save):
    A, B = engine(cfg, n_keys, chunk), engine(cfg, n_keys, chunk)
    fill(A, n_keys, chunk)
    slots = A.limiter_slots(0)
    regions = slots // rl_amd.REGION_SLOTS
    table_bytes = slots * (40 if "local_cache_ttl_ms" in cfg else 32)
    s = torch.cuda.Stream()
    cap = n_keys + 4096
    out = torch.zeros(cap * 6, dtype=torch.int64, device="cuda")
    hdr = torch.zeros(4, dtype=torch.int64, device="cuda")
    src = torch.zeros(table_bytes // 8, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    count = [0]

    def snap():
        # (the header of a call is read before the next one: a call's output starts where the
        # previous one's ended; a table of at most 65536 regions is one call)
        at = n = 0
        while at < regions:
            A.snapshot_keys_device(0, at, SNAP_REGIONS, out[6 * n:], cap - n, hdr, s.cuda_stream)
            if regions <= SNAP_REGIONS:
                at = regions
            else:
                s.synchronize()
                h = hdr.cpu()
                n, at = n + int(h[0]), at + int(h[1])
        count[0] = n

    res = {"case": name, "keys": n_keys, "slots": slots, "table_MB": round(table_bytes / 1e6, 1)}
    res["snapshot_device_ms"] = timed_stream(reps, s, snap)
    s.synchronize()
    if regions <= SNAP_REGIONS:
        count[0] = int(hdr.cpu()[0])
    n = count[0]
    assert n == n_keys, (n, n_keys)
    res["images"] = n
    res["image_MB"] = round(n * 48 / 1e6, 1)
    res["put_device_ms"] = timed_stream(reps, s, lambda: B.put_keys_device(n, out, hdr, s.cuda_stream))
    s.synchronize()
    assert [int(x) for x in hdr.cpu()] == [n, 0, 0, n]
    with torch.cuda.stream(s):
        res["d2d_copy_ms"] = timed_stream(reps, s, lambda: dst.copy_(src, non_blocking=True))
    imgs = out[:6 * n].cpu().numpy().view(rl_amd.KEY_IMAGE_DTYPE)
    # the host forms, chunk images per call / piece
    C = engine(cfg, n_keys, chunk)
    res["snapshot_host_ms"] = timed_host(reps, lambda: sum(c.shape[0] for c in A.snapshot(0, chunk=chunk)))
    res["restore_host_ms"] = timed_host(reps, lambda: C.restore_keys(imgs))
    assert C.limiter_usage(0, T0 * NS)["live_keys"] == B.limiter_usage(0, T0 * NS)["live_keys"] == n_keys
    if save:
        np.save(save, imgs)
    for e in (A, B, C):
        e.close()
    return res


def part_ref(name, cfg, n_keys, reps, chunk, save):
    A, B = engine(cfg, n_keys, chunk), engine(cfg, n_keys, chunk)
    fill(A, n_keys, chunk)
    imgs = np.load(save)
    res = {"case": name, "lib": rl_amd.LIB_PATH}
    ex = np.zeros(2 * n_keys + 1024, rl_amd.STATE_DTYPE)
    n_ex = ctypes.c_size_t(0)

    def export():
        st = A._L.rl_export_state(A.handle, (T0 + 1) * NS, ex.ctypes.data_as(ctypes.c_void_p), ex.shape[0],
                                  ctypes.byref(n_ex))
        assert st == rl_amd.RL_OK and n_ex.value == n_keys, (st, n_ex.value)

    res["export_state_ms"] = timed_host(reps, export)
    res["put_keys_ms"] = timed_host(reps, lambda: B.put_keys(imgs))
    for e in (A, B):
        e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--cases", nargs="+", default=list(ALGOS), choices=list(ALGOS))
    ap.add_argument("--part", default="all", choices=["all", "new", "ref"])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--scratch", default=os.environ.get("TMPDIR", "/tmp"))
    a = ap.parse_args()
    for name in a.cases:
        save = os.path.join(a.scratch, f"snapshot_probe_{name}.npy")
        if a.part in ("all", "new"):
            print(json.dumps(part_new(name, ALGOS[name], a.keys, a.reps, a.chunk, save)), flush=True)
        if a.part == "ref":
            print(json.dumps(part_ref(name, ALGOS[name], a.keys, a.reps, a.chunk, save)), flush=True)
        if a.part == "all":                         # a fresh process: another build of the library
            env = dict(os.environ)
            if a.parent_lib:
                env["RL_ENGINE_LIB"] = os.path.abspath(a.parent_lib)
            if a.parent_pkg:
                env["RL_PROBE_PKG"] = os.path.abspath(a.parent_pkg)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--part", "ref", "--cases", name,
                                   "--keys", str(a.keys), "--reps", str(max(a.reps // 2, 2)),
                                   "--chunk", str(a.chunk), "--scratch", a.scratch], env=env)
            os.remove(save)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps}))


if __name__ == "__main__":
    main()
