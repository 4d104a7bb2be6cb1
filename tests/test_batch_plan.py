"""The arithmetic of a batch (csrc/rl_batch_plan.hpp: digit split, routing, tiles, segments, the
k_group tile bound) against brute force and hand-derived points, on the CPU
(tests/cpp/test_batch_plan.cpp)."""
import os
import subprocess

import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_batch_plan")


def test_batch_plan_properties_and_tile_bound():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/test_batch_plan"])
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batch plan: ok" in r.stdout
