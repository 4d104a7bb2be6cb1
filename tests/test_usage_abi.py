"""CPU-side checks of rl_limiter_usage / rl_top_consumers at the C-ABI boundary (no device calls)."""
import ctypes
import re

import numpy as np

import rl_amd

NEW = ["rl_limiter_usage", "rl_top_consumers"]


def test_entry_points_are_exported_and_the_abi_version_is_unchanged():
    L = rl_amd.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert set(NEW) <= set(rl_amd.EXPORTS)
    assert L.rl_abi_version() == 3


def test_constants_and_struct_match_the_header():
    hdr = open(rl_amd.HEADER).read()
    for name, val in (("RL_USAGE_BINS", rl_amd.USAGE_BINS),
                      ("RL_USAGE_CANDIDATES", rl_amd.USAGE_CANDIDATES)):
        m = re.search(rf"#define {name}\s+(\d+)", hdr)
        assert m, name
        assert int(m.group(1)) == val
    assert (rl_amd.USAGE_BINS, rl_amd.USAGE_CANDIDATES) == (16, 65536)
    for name in NEW:
        assert re.search(rf"\b{name}\(", hdr), name
    assert ctypes.sizeof(rl_amd.Usage) == 8 * (7 + 16)
    # the structure's fields, in the header's order
    body = re.search(r"typedef struct rl_usage \{(.*?)\} rl_usage;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"uint64_t\s+(\w+)", body)
    assert fields == [f for f, _ in rl_amd.Usage._fields_]


def test_invalid_arguments_are_rejected_before_any_device_call():
    """A null engine is checked first, so every case runs without a GPU, and nothing is written
    to the outputs."""
    L = rl_amd.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    bad = rl_amd.RL_E_INVALID_ARG
    u = rl_amd.Usage()
    ctypes.memset(ctypes.byref(u), 0x5A, ctypes.sizeof(u))
    before = bytes(u)
    assert L.rl_limiter_usage(None, 0, 0, ctypes.byref(u)) == bad
    assert L.rl_limiter_usage(None, 9, 0, ctypes.byref(u)) == bad       # (an unknown limiter)
    assert L.rl_limiter_usage(None, 0, 0, None) == bad
    assert bytes(u) == before

    keys = np.full(8, 7, np.uint64)
    used = np.full(8, 7, np.int64)
    n_out = ctypes.c_size_t(7)
    n_match = ctypes.c_uint64(7)

    def top(e, lim, k, mu, kh=keys, us=used, no=ctypes.byref(n_out), nm=ctypes.byref(n_match)):
        return L.rl_top_consumers(e, lim, 0, k, mu, None if kh is None else vp(kh),
                                  None if us is None else vp(us), no, nm)

    assert top(None, 0, 4, 1) == bad
    assert top(None, 9, 4, 1) == bad
    for k, mu in ((0, 1), (rl_amd.TOP_KEYS_MAX + 1, 1), (4, -1)):
        assert top(None, 0, k, mu) == bad
    assert top(None, 0, 4, 1, kh=None) == bad
    assert top(None, 0, 4, 1, us=None) == bad
    assert top(None, 0, 4, 1, no=None) == bad
    assert top(None, 0, 4, 1, nm=None) == bad
    assert np.all(keys == 7) and np.all(used == 7)
    assert n_out.value == 7 and n_match.value == 7
