"""CPU-side checks of the retry-after entry points at the C-ABI boundary (no device calls)."""
import ctypes
import re

import numpy as np

import rl_amd


def test_retry_constants_match_header():
    hdr = open(rl_amd.HEADER).read()
    for name, val in (("RL_RETRY_NEVER", rl_amd.RETRY_NEVER), ("RL_RETRY_INVALID", rl_amd.RETRY_INVALID)):
        m = re.search(rf"#define {name}\s+\(?(-?\d+)\)?", hdr)
        assert m, name
        assert int(m.group(1)) == val
    assert (rl_amd.RETRY_NEVER, rl_amd.RETRY_INVALID) == (-1, -2)


def test_entry_points_are_exported_and_the_abi_version_is_unchanged():
    L = rl_amd.lib()
    assert hasattr(L, "rl_retry_after") and hasattr(L, "rl_retry_after_device")
    assert {"rl_retry_after", "rl_retry_after_device"} <= set(rl_amd.EXPORTS)
    assert L.rl_abi_version() == 3


def test_null_engine_and_null_arrays_are_invalid_arguments():
    """Rejected on the host before any device call: this runs without a GPU."""
    L = rl_amd.lib()
    k = np.array([1, 2], np.uint64)
    p = np.array([1, 1], np.int32)
    t = np.array([0, 0], np.int64)
    w = np.full(2, 7, np.int64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert L.rl_retry_after(None, 2, vp(k), vp(p), vp(t), None, None, vp(w)) == rl_amd.RL_E_INVALID_ARG
    assert L.rl_retry_after(None, 2, None, None, None, None, None, None) == rl_amd.RL_E_INVALID_ARG
    assert L.rl_retry_after(None, 0, None, None, None, None, None, None) == rl_amd.RL_E_INVALID_ARG
    assert L.rl_retry_after_device(None, 2, vp(k), vp(p), vp(t), None, None, vp(w), None) == \
        rl_amd.RL_E_INVALID_ARG
    assert L.rl_retry_after_device(None, 2, None, None, None, None, None, None, None) == \
        rl_amd.RL_E_INVALID_ARG
    assert np.all(w == 7)
