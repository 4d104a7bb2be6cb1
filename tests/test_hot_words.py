"""The summary / verdict word format of the hot regions (csrc/rl_hot_words.hpp: the interface
between k_hot_summ, the chains and k_hot_fill) against bit positions written out by hand, on the
CPU (tests/cpp/test_hot_words.cpp)."""
import os
import subprocess

import rl_amd

BIN = os.path.join(rl_amd.PKG_DIR, "bin", "test_hot_words")


def test_hot_words_layout_and_round_trips():
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", rl_amd.PKG_DIR, "bin/test_hot_words"])
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hot words: ok" in r.stdout
