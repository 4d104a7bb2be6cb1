"""The arithmetic of a table shrink (csrc/rl_shrink.hpp: the halvings rule, the pass schedule)
against brute force, on the CPU (tests/cpp/test_shrink_plan.cpp)."""
import os
import subprocess

import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_shrink_plan")


def test_halvings_rule_and_pass_schedule():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/test_shrink_plan"])
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shrink plan: ok" in r.stdout
