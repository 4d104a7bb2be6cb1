"""The arithmetic of a string-key batch (csrc/rl_keys.hpp: the offset check, the chunk planner)
against brute force, on the CPU (tests/cpp/test_keys_plan.cpp)."""
import os
import subprocess

import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_keys_plan")


def test_offset_check_and_chunk_planner():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/test_keys_plan"])
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "keys plan: ok" in r.stdout
