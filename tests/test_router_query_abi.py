"""CPU-side checks of the router's operation and retry-after entry points at the C-ABI boundary
(rl_router_execute, rl_router_retry_after and the four rl_route_* helpers; no device calls)."""
import ctypes
import re

import numpy as np

import rl_amd

NEW = ("rl_router_execute", "rl_router_retry_after", "rl_route_partition_skip_device",
       "rl_route_fold_ops", "rl_route_unfold_ops", "rl_route_unpack_wait")


def test_the_six_entry_points_are_exported_and_listed():
    L = rl_amd.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert set(NEW) <= set(rl_amd.EXPORTS)
    assert L.rl_abi_version() == 3


def test_retry_error_matches_header():
    hdr = open(rl_amd.HEADER).read()
    m = re.search(r"#define RL_RETRY_ERROR\s+\(?(-?\d+)\)?", hdr)
    assert m and int(m.group(1)) == rl_amd.RETRY_ERROR == -3
    assert re.search(r"#define RL_ABI_VERSION\s+3\b", hdr)
    assert len({rl_amd.RETRY_NEVER, rl_amd.RETRY_INVALID, rl_amd.RETRY_ERROR}) == 3


def test_null_router_or_engine_is_an_invalid_argument():
    """Rejected on the host before any device call, outputs untouched: this runs without a GPU."""
    L = rl_amd.lib()
    n = 3
    k = np.array([1, 2, 3], np.uint64)
    p = np.ones(n, np.int32)
    t = np.zeros(n, np.int64)
    lim = np.zeros(n, np.uint16)
    op = np.zeros(n, np.uint8)
    a = np.full(n, 9, np.uint8)
    r = np.full(n, 7, np.int64)
    w = np.full(n, 7, np.int64)
    perm = np.full(n, 5, np.uint32)
    col = np.full(n, 11, np.uint16)
    cnt = np.full(8, 13, np.int64)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    bad = rl_amd.RL_E_INVALID_ARG
    assert L.rl_router_execute(None, n, vp(k), vp(p), vp(t), vp(lim), vp(op), vp(a), vp(r), None) == bad
    assert L.rl_router_execute(None, 0, None, None, None, None, None, None, None, None) == bad
    assert L.rl_router_retry_after(None, n, vp(k), vp(p), vp(t), vp(lim), vp(a), vp(w), None) == bad
    assert L.rl_router_retry_after(None, 0, None, None, None, None, None, None, None) == bad
    assert L.rl_route_partition_skip_device(None, n, vp(k), vp(a), 2, vp(perm), vp(cnt), 1, None) == bad
    assert L.rl_route_fold_ops(None, n, vp(perm), vp(lim), vp(op), vp(col), None) == bad
    assert L.rl_route_unfold_ops(None, n, vp(col), vp(lim), vp(op), None) == bad
    assert L.rl_route_unpack_wait(None, n, n, vp(perm), vp(r), vp(a), vp(w), None) == bad
    assert np.all(a == 9) and np.all(r == 7) and np.all(w == 7)
    assert np.all(perm == 5) and np.all(col == 11) and np.all(cnt == 13)
    assert np.all(lim == 0) and np.all(op == 0)
