"""CPU-side checks of the table-check calls at the C-ABI boundary (no device calls)."""
import ctypes
import re

import numpy as np

import rl_amd

NEW = ["rl_check_limiter", "rl_check_limiter_device", "rl_check_table_device", "rl_check_images",
       "rl_check_images_device"]


def test_entry_points_are_exported_and_the_abi_version_is_unchanged():
    L = rl_amd.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert set(NEW) <= set(rl_amd.EXPORTS)
    assert L.rl_abi_version() == 3


def test_struct_matches_the_header():
    hdr = open(rl_amd.HEADER).read()
    for name in NEW:
        assert re.search(rf"\b{name}\(", hdr), name
    assert ctypes.sizeof(rl_amd.CheckReport) == 8 * (7 + 2 * 16) == 312
    body = re.search(r"typedef struct rl_check_report \{(.*?)\} rl_check_report;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f for decl in re.findall(r"uint64_t\s+([^;]+);", body)
              for f in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl)]
    assert fields == [f for f, _ in rl_amd.CheckReport._fields_]
    d = rl_amd.check_dict(np.arange(rl_amd.CHECK_WORDS, dtype=np.uint64))
    assert d["regions"] == 0 and d["bad_slots"] == 6 and d["violations"][0] == 7 and d["first"][15] == 38


def test_invalid_arguments_are_rejected_before_any_device_call():
    """A null engine is checked first, so every case runs without a GPU, and nothing is written
    to the outputs."""
    L = rl_amd.lib()
    bad = rl_amd.RL_E_INVALID_ARG
    r = rl_amd.CheckReport()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    before = bytes(r)
    rp = ctypes.byref(r)
    raw = ctypes.c_void_p(ctypes.addressof(r))
    imgs = np.zeros(4, rl_amd.KEY_IMAGE_DTYPE)
    ip = imgs.ctypes.data_as(ctypes.c_void_p)
    tab = np.zeros(64, np.uint64).ctypes.data_as(ctypes.c_void_p)

    assert L.rl_check_limiter(None, 0, 0, 8, rp) == bad
    assert L.rl_check_limiter(None, 9, 0, 8, rp) == bad                  # (an unknown limiter)
    assert L.rl_check_limiter(None, 0, 0, 8, None) == bad
    assert L.rl_check_limiter_device(None, 0, 0, 8, raw, None) == bad
    assert L.rl_check_limiter_device(None, 0, 0, 8, None, None) == bad
    assert L.rl_check_limiter_device(None, 0, 0, 8, ctypes.c_void_p(raw.value + 4), None) == bad
    for bits in (0, 2, 3, 24, 25):
        assert L.rl_check_table_device(None, 0, tab, None, bits, raw, None) == bad
    assert L.rl_check_table_device(None, 0, None, None, 3, raw, None) == bad
    assert L.rl_check_table_device(None, 0, ctypes.c_void_p(tab.value + 8), None, 3, raw, None) == bad
    assert L.rl_check_table_device(None, 0, tab, ctypes.c_void_p(tab.value + 4), 3, raw, None) == bad
    assert L.rl_check_table_device(None, 0, tab, None, 3, None, None) == bad
    assert L.rl_check_images(None, 4, ip, rp) == bad
    assert L.rl_check_images(None, 4, None, rp) == bad
    assert L.rl_check_images(None, 4, ip, None) == bad
    assert L.rl_check_images(None, (1 << 31) + 1, ip, rp) == bad         # (the null engine comes first)
    assert L.rl_check_images_device(None, 4, ip, raw, None) == bad
    assert L.rl_check_images_device(None, 4, None, raw, None) == bad
    assert L.rl_check_images_device(None, 4, ctypes.c_void_p(ip.value + 8), raw, None) == bad
    assert L.rl_check_images_device(None, 4, ip, None, None) == bad
    assert bytes(r) == before
