"""CPU-side checks of the top-keys entry points at the C-ABI boundary (no device calls)."""
import ctypes
import re

import numpy as np

import rl_amd

NEW = ["rl_top_keys", "rl_top_keys_device", "rl_router_plan_directory_sampled"]


def test_entry_points_are_exported_and_the_abi_version_is_unchanged():
    L = rl_amd.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert set(NEW) <= set(rl_amd.EXPORTS)
    assert L.rl_abi_version() == 3


def test_constants_match_the_header():
    hdr = open(rl_amd.HEADER).read()
    for name, val in (("RL_TOP_KEYS_MAX", rl_amd.TOP_KEYS_MAX),
                      ("RL_TOP_KEYS_CANDIDATES", rl_amd.TOP_KEYS_CANDIDATES)):
        m = re.search(rf"#define {name}\s+(\d+)", hdr)
        assert m, name
        assert int(m.group(1)) == val
    assert (rl_amd.TOP_KEYS_MAX, rl_amd.TOP_KEYS_CANDIDATES) == (4096, 65536)
    for name in NEW:
        assert re.search(rf"\b{name}\(", hdr), name


def test_invalid_arguments_are_rejected_before_any_device_call():
    """A null engine is checked with the other arguments on the host: this runs without a GPU,
    and nothing is written to the outputs."""
    L = rl_amd.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    keys = np.array([1, 2, 2], np.uint64)
    top = np.full(4, 7, np.uint64)
    cnt = np.full(4, 7, np.uint64)
    hdr = np.full(4, 7, np.uint64)
    n_out = ctypes.c_size_t(7)
    heavy = ctypes.c_uint64(7)
    bad = rl_amd.RL_E_INVALID_ARG

    def host(e, n, k, kk, mc, t=top, c=cnt, no=ctypes.byref(n_out), nh=ctypes.byref(heavy)):
        return L.rl_top_keys(e, n, k, kk, mc, None if t is None else vp(t),
                             None if c is None else vp(c), no, nh)

    def dev(e, n, k, kk, mc, t=top, c=cnt, h=hdr):
        return L.rl_top_keys_device(e, n, k, kk, mc, None if t is None else vp(t),
                                    None if c is None else vp(c), None if h is None else vp(h), None)

    # a null engine, with arguments that are otherwise fine and with each bad one
    assert host(None, 3, vp(keys), 4, 1) == bad
    assert dev(None, 3, vp(keys), 4, 1) == bad
    for k, mc in ((0, 1), (4097, 1), (4, 0)):
        assert host(None, 3, vp(keys), k, mc) == bad
        assert dev(None, 3, vp(keys), k, mc) == bad
    assert host(None, 3, None, 4, 1) == bad and dev(None, 3, None, 4, 1) == bad
    assert host(None, 3, vp(keys), 4, 1, t=None) == bad and dev(None, 3, vp(keys), 4, 1, t=None) == bad
    assert host(None, 3, vp(keys), 4, 1, c=None) == bad and dev(None, 3, vp(keys), 4, 1, c=None) == bad
    assert host(None, 3, vp(keys), 4, 1, no=None) == bad and host(None, 3, vp(keys), 4, 1, nh=None) == bad
    assert dev(None, 3, vp(keys), 4, 1, h=None) == bad
    assert host(None, (1 << 31) + 1, vp(keys), 4, 1) == bad
    assert L.rl_router_plan_directory_sampled(None, 3, vp(keys), 4, 1, None, None) == bad
    assert np.all(top == 7) and np.all(cnt == 7) and np.all(hdr == 7)
    assert n_out.value == 7 and heavy.value == 7
