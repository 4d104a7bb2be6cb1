"""The predicates of the table check (csrc/rl_check.hpp) against brute force on crafted 256-slot
regions, on the CPU (tests/cpp/test_check_plan.cpp; once more built with the address and
undefined-behaviour sanitizers, a stand-alone host program), and the constants the Python model
(check_cases.py) and the package share with the header."""
import os
import re
import subprocess

import check_cases as cc
import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_check_plan")
HPP = os.path.join(rl_amd.PKG_DIR, "csrc", "rl_check.hpp")


def run_plan(binary):
    subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/" + os.path.basename(binary)])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"check plan: ok \((\d+) regions\) classes=(\d+) slots=(\d+) dead_mark=(\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    return [int(x) for x in m.groups()]


def test_predicates_against_brute_force():
    regions, classes, slots, dead = run_plan(BIN)
    assert regions == 2 + 256 + 7 + 15 * 4
    assert (classes, slots, dead) == (cc.CLASSES, cc.NS, cc.DEAD)


def test_predicates_under_sanitizers():
    assert run_plan(BIN + "_san")[1] == cc.CLASSES


def test_class_ids_agree_everywhere():
    """rl_check.hpp's enum, the header's RL_CHECK_* and the two Python restatements."""
    hpp = open(HPP).read()
    hdr = open(rl_amd.HEADER).read()
    names = {"WRONG_REGION": "kCkWrongRegion", "UNREACHABLE": "kCkUnreachable", "DUPLICATE": "kCkDuplicate",
             "DEAD_MARK": "kCkDeadMark", "SW_START": "kCkSwStart", "SW_COUNT": "kCkSwCount",
             "SW_OFFSET": "kCkSwOffset", "TB_FLAGS": "kCkTbFlags", "TB_TOKENS": "kCkTbTokens",
             "IMAGE_LIMITER": "kCkImageLimiter", "IMAGE_RESERVED": "kCkImageReserved"}
    for name, k in names.items():
        h = int(re.search(rf"#define RL_CHECK_{name}\s+(\d+)", hdr).group(1))
        c = int(re.search(rf"\b{k} = (\d+)", hpp).group(1))
        assert h == c == getattr(cc, name) == getattr(rl_amd, "CHECK_" + name), name
    assert int(re.search(r"#define RL_CHECK_CLASSES\s+(\d+)", hdr).group(1)) == cc.CLASSES == rl_amd.CHECK_CLASSES
    assert rl_amd.DEAD_MARK == cc.DEAD and rl_amd.CHECK_NONE == cc.NONE
