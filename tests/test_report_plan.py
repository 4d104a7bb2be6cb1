"""The batch report's row / class rule (csrc/rl_report.hpp) against the hand-written table of
tests/cpp/test_report_plan.cpp, and the numpy restatement the GPU tests use against the same
corners. CPU only."""
import os
import subprocess

import numpy as np

import report_cases as rc
import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_report_plan")


def test_report_plan():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/test_report_plan"])
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "report_plan: ok (675 cases)" in r.stdout


def test_the_numpy_restatement_on_a_batch_counted_by_hand():
    """Seven limiters known. One request per line below."""
    #        permits limiter op  allowed remaining   row  class
    rows = [(1,      0,      0,  1,      4),       # 0    allowed
            (2,      0,      0,  0,      0),       # 0    denied
            (9,      0,      0,  0,      -1),      # 0    denied, over max
            (1,      0,      0,  0,      -3),      # 0    error
            (1,      0,      0,  0,      -2),      # 0    denied (a regressed bucket's balance)
            (0,      0,      0,  0,      -2),      # 0    invalid (permits)
            (0,      0,      1,  1,      3),       # 0    peek (permits are not looked at)
            (1,      6,      2,  1,      0),       # 6    reset
            (1,      7,      0,  0,      -2),      # 255  invalid (limiter == L)
            (1,      65535,  1,  1,      5),       # 255  invalid
            (1,      6,      3,  1,      5),       # 6    invalid (no such op)
            (2147483647, 6,  0,  2,      1)]       # 6    allowed (any non-zero `allowed`)
    a = [np.array(c) for c in zip(*rows)]
    t = rc.tally_model(7, a[0].astype(np.int32), a[1].astype(np.uint16), a[2].astype(np.uint8),
                       a[3].astype(np.uint8), a[4].astype(np.int64))
    want = {0: dict(requests=7, invalid=1, errors=1, allowed=1, denied=3, over_max=1, peeks=1, resets=0,
                    permits_allowed=1, permits_denied=12),
            6: dict(requests=3, invalid=1, errors=0, allowed=1, denied=0, over_max=0, peeks=0, resets=1,
                    permits_allowed=2147483647, permits_denied=0),
            255: dict(requests=2, invalid=2, errors=0, allowed=0, denied=0, over_max=0, peeks=0, resets=0,
                      permits_allowed=0, permits_denied=0)}
    for r in range(rl_amd.TALLY_ROWS):
        for f in rl_amd.TALLY_DTYPE.names[:10]:
            assert int(t[f][r]) == want.get(r, {}).get(f, 0), (r, f)
    # limiter and op absent: limiter 0, ACQUIRE
    t0 = rc.tally_model(7, a[0].astype(np.int32), None, None, a[3].astype(np.uint8), a[4].astype(np.int64))
    assert int(t0["requests"][0]) == 12 and int(t0["requests"][1:].sum()) == 0
    assert int(t0["peeks"][0]) == 0 and int(t0["invalid"][0]) == 2
    keys = np.array([5, 9, 9, 9, 9, 1, 1, 2, 9, 9, 9, 9], np.uint64)
    tk, tc, heavy, denied = rc.top_denied_model(7, keys, *[x for x in (a[0], a[1], a[2], a[3], a[4])], 0, 4, 1)
    assert (list(tk), list(tc), heavy, denied) == ([9], [3], 1, 3)
