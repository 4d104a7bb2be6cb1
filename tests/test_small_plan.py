"""The small-batch path's stable partition by region run on the host through the functions of
csrc/rl_small.hpp (tests/cpp/test_small_plan.cpp): four region patterns (one region, all distinct,
two alternating, descending) at eleven sizes against std::stable_sort, in buffers of exactly the
sizes the header states; once more built with the address and undefined-behaviour sanitizers (a
stand-alone host program). The constants it prints are checked against the headers."""
import os
import re
import subprocess

import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_small_plan")
SIZES = 11                                     # 0, 1, 2, 63..65, 255..257, MAX - 1, MAX
PATTERNS = 4


def run_plan(binary):
    subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/" + os.path.basename(binary)])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"small plan: ok \((\d+) cases\) (.*)", r.stdout)
    assert m, r.stdout + r.stderr
    return int(m.group(1)), {k: int(v) for k, v in (kv.split("=") for kv in m.group(2).split())}


def header_constant(name):
    src = open(os.path.join(rl_amd.PKG_DIR, "csrc", "rl_small.hpp")).read()
    return int(re.search(rf"constexpr uint32_t {name} = (\d+);", src).group(1))


def test_partition_against_stable_sort():
    cases, c = run_plan(BIN)
    assert cases == PATTERNS * SIZES
    assert c["max"] == header_constant("kSmallMax") == rl_amd.SMALL_BATCH_MAX >= 1024
    abi = int(re.search(r"#define RL_SMALL_BATCH_MAX (\d+)", open(rl_amd.HEADER).read()).group(1))
    assert abi == c["max"]
    assert c["threads"] == header_constant("kSmallThreads") and c["threads"] % 64 == 0
    assert c["waves"] * 64 == c["threads"] and c["per"] * c["threads"] == c["max"]
    # key, now, remaining, tokens (8 B), permits (4), limiter (2), op, allowed (1) per request
    assert c["block_bytes"] == c["max"] * (4 * 8 + 4 + 2 + 1 + 1)


def test_partition_under_sanitizers():
    cases, c = run_plan(BIN + "_san")
    assert cases == PATTERNS * SIZES and c["max"] == rl_amd.SMALL_BATCH_MAX
