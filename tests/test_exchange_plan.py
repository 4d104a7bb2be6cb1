"""The round plan of a router exchange (csrc/rl_exchange.hpp: rounds, per-pair send and receive
ranges from the count matrix, the receive capacity and the rank) against brute force, on the CPU
(tests/cpp/test_exchange_plan.cpp): G in {1, 2, 4, 8}, random matrices with zero rows and
columns, capacities 1, one that divides evenly and one that does not."""
import os
import subprocess

import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_exchange_plan")


def test_round_plan_matches_brute_force():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/test_exchange_plan"])
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok (0 failures)" in r.stdout and "exchange plan:" in r.stdout
