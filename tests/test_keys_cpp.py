"""String-key batches through the C++ mirror: KeyBatch, GpuEngine::hashKeys and
GpuRateLimiter::tryAcquireBatch(KeyBatch, ...) against the per-call string path
(tests/cpp/test_keys.cpp)."""
import os
import subprocess

import pytest

import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_keys")


@pytest.mark.gpu
def test_key_batches_through_the_host_api():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR])
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "keys: ok" in r.stdout
