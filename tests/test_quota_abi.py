"""CPU-side checks of the quota entry points at the C-ABI boundary (no device calls)."""
import ctypes
import re

import numpy as np

import rl_amd


def test_quota_constant_matches_header():
    hdr = open(rl_amd.HEADER).read()
    m = re.search(r"#define RL_QUOTA_INVALID\s+\(?(-?\d+)\)?", hdr)
    assert m and int(m.group(1)) == rl_amd.QUOTA_INVALID == -2


def test_entry_points_are_exported_and_the_abi_version_is_unchanged():
    L = rl_amd.lib()
    assert hasattr(L, "rl_quota") and hasattr(L, "rl_quota_device")
    assert {"rl_quota", "rl_quota_device"} <= set(rl_amd.EXPORTS)
    hdr = open(rl_amd.HEADER).read()
    assert re.search(r"\bint\s+rl_quota\(", hdr) and re.search(r"\bint\s+rl_quota_device\(", hdr)
    assert L.rl_abi_version() == 3


def test_null_engine_null_arrays_and_mismatched_arguments_are_invalid_arguments():
    """Rejected on the host before any device call: this runs without a GPU."""
    L = rl_amd.lib()
    k = np.array([1, 2], np.uint64)
    t = np.array([0, 0], np.int64)
    p = np.array([1, 1], np.int32)
    sk = np.zeros(2, np.uint8)
    rem, rst, rty = (np.full(2, 7, np.int64) for _ in range(3))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    bad = rl_amd.RL_E_INVALID_ARG
    # a NULL engine, with everything else in order
    assert L.rl_quota(None, 2, vp(k), vp(t), None, vp(p), None, vp(rem), vp(rst), vp(rty)) == bad
    assert L.rl_quota(None, 2, vp(k), vp(t), None, None, None, vp(rem), vp(rst), None) == bad
    assert L.rl_quota(None, 0, None, None, None, None, None, None, None, None) == bad
    # NULL arrays
    assert L.rl_quota(None, 2, None, None, None, None, None, None, None, None) == bad
    assert L.rl_quota(None, 2, vp(k), vp(t), None, None, None, None, vp(rst), None) == bad
    assert L.rl_quota(None, 2, vp(k), vp(t), None, None, None, vp(rem), None, None) == bad
    # permits without retry_ms, retry_ms without permits, skip without permits
    assert L.rl_quota(None, 2, vp(k), vp(t), None, vp(p), None, vp(rem), vp(rst), None) == bad
    assert L.rl_quota(None, 2, vp(k), vp(t), None, None, None, vp(rem), vp(rst), vp(rty)) == bad
    assert L.rl_quota(None, 2, vp(k), vp(t), None, None, vp(sk), vp(rem), vp(rst), None) == bad
    # the device form
    assert L.rl_quota_device(None, 2, vp(k), vp(t), None, vp(p), None, vp(rem), vp(rst), vp(rty), None) == bad
    assert L.rl_quota_device(None, 2, None, None, None, None, None, None, None, None, None) == bad
    assert L.rl_quota_device(None, 2, vp(k), vp(t), None, vp(p), None, vp(rem), vp(rst), None, None) == bad
    assert np.all(rem == 7) and np.all(rst == 7) and np.all(rty == 7)
