"""Mixed operations and retry-after queries through the C-ABI router (rl_router_execute,
rl_router_retry_after) driven from C++ (tests/cpp/test_router_query.cpp): G = 2 / 4 / 8 routers as
threads on the box's GPU over the in-process transport, every decision and every wait equal to
one unsharded engine's on the concatenated stream; one subprocess per mode."""
import os
import subprocess

import pytest

import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_router_query")

pytestmark = pytest.mark.gpu


def _run(mode):
    r = subprocess.run([BIN, mode], capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{mode}: ok (0 failures)" in r.stdout, r.stdout
    return r.stdout


def test_execute_with_ops_equals_one_engine():
    out = _run("execute")
    assert out.count(" 0 mismatches") == 7 and out.count(" 0 wait mismatches") == 7, out


def test_retry_after_equals_one_engine_in_every_exchange_mode():
    out = _run("retry")
    assert out.count(" 0 mismatches") == 4 and out.count(" 0 wait mismatches") == 4, out


def test_execute_and_retry_after_at_eight_shards():
    out = _run("shards")
    assert out.count(" 0 mismatches") == 2 and out.count(" 0 wait mismatches") == 2, out


def test_capacity_mismatch_fails_every_rank():
    _run("mismatch")
