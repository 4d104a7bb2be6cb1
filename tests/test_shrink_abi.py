"""CPU-side checks of rl_shrink_plan / rl_shrink_limiter at the C-ABI boundary (no device calls)."""
import ctypes
import re

import rl_amd

NEW = ["rl_shrink_plan", "rl_shrink_limiter"]


def test_entry_points_are_exported_and_the_abi_version_is_unchanged():
    L = rl_amd.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert set(NEW) <= set(rl_amd.EXPORTS)
    assert L.rl_abi_version() == 3
    assert re.search(r"#define RL_ABI_VERSION\s+3\b", open(rl_amd.HEADER).read())


def test_constants_and_struct_match_the_header():
    hdr = open(rl_amd.HEADER).read()
    for name, val in (("RL_SHRINK_FILL_MAX", rl_amd.SHRINK_FILL_MAX),
                      ("RL_SHRINK_LEVELS", rl_amd.SHRINK_LEVELS)):
        m = re.search(rf"#define {name}\s+(\d+)", hdr)
        assert m, name
        assert int(m.group(1)) == val
    assert (rl_amd.SHRINK_FILL_MAX, rl_amd.SHRINK_LEVELS) == (104, 24)
    for name in NEW:
        assert re.search(rf"\b{name}\(", hdr), name
    assert ctypes.sizeof(rl_amd.ShrinkReport) == 8 * 4 + 4 * 2 + 4 * 24
    # the structure's fields, in the header's order and with the header's types
    body = re.search(r"typedef struct rl_shrink_report \{(.*?)\} rl_shrink_report;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint64_t|uint32_t)\s+(\w+)(\[RL_SHRINK_LEVELS\])?\s*;", body)
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    want = [(n, ctype[t] * rl_amd.SHRINK_LEVELS if arr else ctype[t]) for t, n, arr in fields]
    assert [n for n, _ in want] == ["slots_before", "slots_after", "used_before", "kept", "halvings",
                                    "levels", "fullest"]
    assert want == list(rl_amd.ShrinkReport._fields_)
    # the fill bound is half the fill at which a batch flags growth (kGrowUsed, rl_launch.hpp)
    src = open(rl_amd.PKG_DIR + "/csrc/rl_launch.hpp").read()
    grow = int(re.search(r"constexpr uint32_t kGrowUsed = (\d+);", src).group(1))
    assert 2 * rl_amd.SHRINK_FILL_MAX == grow


def test_invalid_arguments_are_rejected_before_any_device_call():
    """A null engine is checked first, so every case runs without a GPU, and nothing is written
    to the outputs."""
    L = rl_amd.lib()
    bad = rl_amd.RL_E_INVALID_ARG
    r = rl_amd.ShrinkReport()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    before = bytes(r)
    for fn in (L.rl_shrink_plan, L.rl_shrink_limiter):
        assert fn(None, 0, 0, 0, ctypes.byref(r)) == bad
        assert fn(None, 9, 0, 0, ctypes.byref(r)) == bad             # (an unknown limiter)
        assert fn(None, 0, 0, 1 << 40, ctypes.byref(r)) == bad
        assert fn(None, 0, 0, 0, None) == bad                        # null out (required by the plan)
    assert bytes(r) == before
