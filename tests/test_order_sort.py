"""A stable radix sort of a batch by time run on the host through the addressing helpers of
csrc/rl_order.hpp (tests/cpp/test_order_sort.cpp): every timestamp pattern of tests/order_cases.py
at fourteen sizes and one more with a two-step row scan, against std::stable_sort, in buffers of
exactly the sizes the helpers state; once more built with the address and undefined-behaviour
sanitizers (a stand-alone host program). The constants it prints are checked against the header
and against the numpy model's."""
import os
import re
import subprocess

import order_cases as oc
import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_order_sort")
SIZES = 14                                     # 0, 1, 2, 63..65, 511..513, T - 1, T, T + 1, 2T + 17, 40T + 3


def run_sort(binary):
    subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/" + os.path.basename(binary)])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"order sort: ok \((\d+) cases\) (.*)", r.stdout)
    assert m, r.stdout + r.stderr
    return int(m.group(1)), {k: int(v) for k, v in (kv.split("=") for kv in m.group(2).split())}


def header_constant(name):
    src = open(os.path.join(rl_amd.PKG_DIR, "csrc", "rl_order.hpp")).read()
    return int(re.search(rf"constexpr uint32_t {name} = (\d+);", src).group(1))


def test_sort_against_stable_sort():
    cases, c = run_sort(BIN)
    assert cases == len(oc.PATTERNS) * SIZES + 1
    assert c["threads"] == header_constant("kOrderThreads") and c["rounds"] == header_constant("kOrderRounds")
    assert c["tile"] == c["threads"] * c["rounds"] and c["threads"] % 64 == 0
    assert c["bins"] == 1 << oc.DIGIT_BITS
    assert c["scan_width"] == header_constant("kOrderScanWidth")
    assert c["two_step_n"] == c["scan_width"] * c["tile"] + 1
    # bytes per request: two (uint64 key, uint32 index) sets; key, permits, now, limiter, op gathered;
    # allowed, remaining, tokens in sorted order
    assert (c["sort_bytes"], c["gather_bytes"], c["result_bytes"]) == (2 * 12, 8 + 4 + 8 + 2 + 1, 1 + 8 + 8)


def test_sort_under_sanitizers():
    cases, c = run_sort(BIN + "_san")
    assert cases == len(oc.PATTERNS) * SIZES + 1 and c["bins"] == 1 << oc.DIGIT_BITS
