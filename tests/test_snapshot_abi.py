"""CPU-side checks of the snapshot / restore entry points at the C-ABI boundary (no device calls):
rl_snapshot_keys(_device), rl_put_keys_device, rl_restore_keys."""
import ctypes
import re

import numpy as np

import rl_amd

NEW = ["rl_snapshot_keys", "rl_snapshot_keys_device", "rl_put_keys_device", "rl_restore_keys"]


def test_entry_points_are_declared_listed_and_exported():
    L = rl_amd.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(rl_amd.HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in rl_amd.EXPORTS, name
        assert hasattr(L, name), name
    assert L.rl_abi_version() == 3
    assert re.search(r"#define RL_ABI_VERSION\s+3\b", hdr)


def test_min_cap_is_one_region():
    hdr = open(rl_amd.HEADER).read()
    m = re.search(r"#define RL_SNAPSHOT_MIN_CAP\s+(\d+)", hdr)
    assert m and int(m.group(1)) == rl_amd.SNAPSHOT_MIN_CAP == rl_amd.REGION_SLOTS == 256
    assert (rl_amd.PUT_REJECT_ORDER, rl_amd.PUT_REJECT_LIMITER) == (1, 2)


def test_a_null_engine_is_rejected_before_any_device_call():
    """The handle is checked first, so every case runs without a GPU and writes nothing."""
    L = rl_amd.lib()
    bad = rl_amd.RL_E_INVALID_ARG
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    imgs = np.zeros(8, rl_amd.KEY_IMAGE_DTYPE)
    imgs.view(np.uint8)[:] = 0xA5
    hdr = np.full(4, 7, np.uint64)
    before = imgs.tobytes()
    n = ctypes.c_size_t(7)
    done, total = ctypes.c_uint64(7), ctypes.c_uint64(7)
    rn, rd, rt = ctypes.byref(n), ctypes.byref(done), ctypes.byref(total)
    assert L.rl_snapshot_keys(None, 0, 0, 8, vp(imgs), 8, rn, rd, rt) == bad
    assert L.rl_snapshot_keys(None, 0, 0, 0, None, 0, rn, rd, rt) == bad
    assert L.rl_snapshot_keys(None, 0, 0, 8, None, 8, rn, rd, rt) == bad
    assert L.rl_snapshot_keys(None, 0, 0, 8, vp(imgs), 8, None, rd, rt) == bad
    assert L.rl_snapshot_keys(None, 0, 0, 8, vp(imgs), 8, rn, None, rt) == bad
    assert L.rl_snapshot_keys(None, 0, 0, 8, vp(imgs), 8, rn, rd, None) == bad
    assert L.rl_snapshot_keys(None, 9, 1 << 40, 1 << 40, vp(imgs), 8, rn, rd, rt) == bad
    assert L.rl_snapshot_keys_device(None, 0, 0, 8, vp(imgs), 8, vp(hdr), None) == bad
    assert L.rl_snapshot_keys_device(None, 0, 0, 8, vp(imgs), 8, None, None) == bad
    assert L.rl_snapshot_keys_device(None, 0, 0, 8, None, 8, vp(hdr), None) == bad
    assert L.rl_snapshot_keys_device(None, 0, 0, 0, None, 0, vp(hdr), None) == bad
    assert L.rl_put_keys_device(None, 8, vp(imgs), vp(hdr), None) == bad
    assert L.rl_put_keys_device(None, 8, None, vp(hdr), None) == bad
    assert L.rl_put_keys_device(None, 8, vp(imgs), None, None) == bad
    assert L.rl_put_keys_device(None, 0, None, vp(hdr), None) == bad
    assert L.rl_restore_keys(None, 8, vp(imgs), rn) == bad
    assert L.rl_restore_keys(None, 8, None, rn) == bad
    assert L.rl_restore_keys(None, 0, None, None) == bad
    assert (n.value, done.value, total.value) == (7, 7, 7)
    assert imgs.tobytes() == before and np.all(hdr == 7)
