"""The digit plan of a sort of a batch by time (csrc/rl_order.hpp) against brute force, on the
CPU (tests/cpp/test_order_plan.cpp; once more built with the address and undefined-behaviour
sanitizers, a stand-alone host program), and the numpy restatement (order_cases.plan_model)
against the same rule and the same constants."""
import os
import re
import subprocess

import order_cases as oc
import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_order_plan")


def run_plan(binary):
    subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/" + os.path.basename(binary)])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"order plan: ok \((\d+) spans\) digit_bits=(\d+) max_passes=(\d+) clock_passes=(\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    return [int(x) for x in m.groups()]


def test_plan_against_brute_force():
    spans, digit_bits, max_passes, clock_passes = run_plan(BIN)
    assert spans == 2 + 3 * 63 + 1
    assert (digit_bits, max_passes, clock_passes) == (oc.DIGIT_BITS, -(-64 // oc.DIGIT_BITS), -(-45 // oc.DIGIT_BITS))


def test_plan_under_sanitizers():
    assert run_plan(BIN + "_san")[1] == oc.DIGIT_BITS


def test_the_numpy_plan_follows_the_same_rule():
    assert oc.plan_model(0) == (0, False, [])
    assert oc.plan_model(1) == (1, False, [(0, 1)])
    assert oc.plan_model(255) == (1, False, [(0, 8)])
    assert oc.plan_model(256) == (2, False, [(0, 5), (5, 4)])
    assert oc.plan_model(3499) == (2, False, [(0, 6), (6, 6)])
    assert oc.plan_model((1 << 32) - 1) == (4, False, [(0, 8), (8, 8), (16, 8), (24, 8)])
    assert oc.plan_model(1 << 32) == (5, True, [(0, 7), (7, 7), (14, 7), (21, 6), (27, 6)])
    for k in range(1, 45):
        for span in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            passes, wide, digits = oc.plan_model(span)
            assert passes == oc.plan_passes(span) == -(-span.bit_length() // 8) <= 6
            assert wide == (span.bit_length() > 32)
            assert sum(b for _, b in digits) == span.bit_length()
            assert all(s == sum(b for _, b in digits[:i]) for i, (s, _) in enumerate(digits))
