"""The arithmetic of a snapshot / ordered put (csrc/rl_snapshot.hpp: the cut rule, the ordered-form
predicate) against brute force, on the CPU (tests/cpp/test_snapshot_plan.cpp)."""
import os
import subprocess

import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_snapshot_plan")


def test_cut_rule_and_ordered_form():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/test_snapshot_plan"])
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "snapshot plan: ok" in r.stdout
