"""CPU-side checks of the key-migration entry points at the C-ABI boundary (no device calls):
rl_copy_keys / rl_drop_keys / rl_put_keys and rl_router_replan_directory(_sampled)."""
import ctypes
import re

import numpy as np

import rl_amd

NEW = ["rl_copy_keys", "rl_drop_keys", "rl_put_keys",
       "rl_router_replan_directory", "rl_router_replan_directory_sampled"]


def test_entry_points_are_declared_listed_and_exported():
    L = rl_amd.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(rl_amd.HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in rl_amd.EXPORTS, name
        assert hasattr(L, name), name
    assert L.rl_abi_version() == 3


def test_constants_and_struct_match_the_header():
    hdr = open(rl_amd.HEADER).read()
    m = re.search(r"#define RL_MOVE_KEYS_MAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == rl_amd.MOVE_KEYS_MAX == 8192
    assert ctypes.sizeof(rl_amd.KeyImage) == 48
    assert rl_amd.KEY_IMAGE_DTYPE.itemsize == 48
    body = re.search(r"typedef struct rl_key_image \{(.*?)\} rl_key_image;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"uint(?:64|16)_t\s+(\w+)", body)
    assert fields == [f for f, _ in rl_amd.KeyImage._fields_] == list(rl_amd.KEY_IMAGE_DTYPE.names)
    for f, _ in rl_amd.KeyImage._fields_:
        assert getattr(rl_amd.KeyImage, f).offset == rl_amd.KEY_IMAGE_DTYPE.fields[f][1], f


def test_a_null_engine_or_router_is_rejected_before_any_device_call():
    """The handle is checked first, so every case runs without a GPU and writes nothing."""
    L = rl_amd.lib()
    bad = rl_amd.RL_E_INVALID_ARG
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    keys = np.full(4, 7, np.uint64)
    imgs = np.zeros(4, rl_amd.KEY_IMAGE_DTYPE)
    imgs["key_hash"] = 7
    before = imgs.tobytes()
    n = ctypes.c_size_t(7)
    n64 = ctypes.c_uint64(7)
    assert L.rl_copy_keys(None, 4, vp(keys), vp(imgs), 4, ctypes.byref(n)) == bad
    assert L.rl_copy_keys(None, 0, None, None, 0, ctypes.byref(n)) == bad
    assert L.rl_copy_keys(None, rl_amd.MOVE_KEYS_MAX + 1, vp(keys), vp(imgs), 4, ctypes.byref(n)) == bad
    assert L.rl_copy_keys(None, 4, None, vp(imgs), 4, ctypes.byref(n)) == bad
    assert L.rl_copy_keys(None, 4, vp(keys), vp(imgs), 4, None) == bad
    assert L.rl_copy_keys(None, 4, vp(keys), None, 4, ctypes.byref(n)) == bad
    assert L.rl_drop_keys(None, 4, vp(keys), ctypes.byref(n64)) == bad
    assert L.rl_drop_keys(None, 4, vp(keys), None) == bad
    assert L.rl_drop_keys(None, 4, None, ctypes.byref(n64)) == bad
    assert L.rl_put_keys(None, 4, vp(imgs), ctypes.byref(n)) == bad
    assert L.rl_put_keys(None, 4, None, ctypes.byref(n)) == bad
    assert n.value == 7 and n64.value == 7
    assert imgs.tobytes() == before and np.all(keys == 7)

    cnt = np.full(4, 3, np.uint64)
    placed = ctypes.c_uint32(7)
    assert L.rl_router_replan_directory(None, 4, vp(keys), vp(cnt), 12, 4, ctypes.byref(placed),
                                        ctypes.byref(n64), None) == bad
    assert L.rl_router_replan_directory(None, 0, None, None, 0, 0, None, None, None) == bad
    assert L.rl_router_replan_directory_sampled(None, 0, None, 4, 1, ctypes.byref(placed),
                                                ctypes.byref(n64), None) == bad
    assert placed.value == 7 and n64.value == 7
