"""The host arithmetic of a directory re-plan (csrc/rl_replan.hpp: mover list, images grouped by
new owner) against brute force, on the CPU (tests/cpp/test_replan_plan.cpp)."""
import os
import subprocess

import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_replan_plan")


def test_mover_list_and_grouping():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/test_replan_plan"])
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "replan plan: ok" in r.stdout
