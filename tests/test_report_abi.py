"""CPU-side checks of rl_tally_batch / rl_top_denied at the C-ABI boundary (no device calls)."""
import ctypes
import re

import numpy as np

import rl_amd

NEW = ["rl_tally_batch", "rl_tally_batch_device", "rl_top_denied", "rl_top_denied_device"]


def test_entry_points_are_exported_and_the_abi_version_is_unchanged():
    L = rl_amd.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert set(NEW) <= set(rl_amd.EXPORTS)
    assert L.rl_abi_version() == 3
    hdr = open(rl_amd.HEADER).read()
    assert re.search(r"#define RL_ABI_VERSION\s+3\b", hdr)
    for name in NEW:
        assert re.search(rf"\b{name}\(", hdr), name


def test_constants_and_the_struct_match_the_header():
    hdr = open(rl_amd.HEADER).read()
    for name, val in (("RL_TALLY_ROWS", rl_amd.TALLY_ROWS), ("RL_TALLY_UNKNOWN", rl_amd.TALLY_UNKNOWN)):
        m = re.search(rf"#define {name}\s+(\d+)", hdr)
        assert m and int(m.group(1)) == val, name
    m = re.search(r"#define RL_TALLY_ACCUMULATE\s+0x([0-9a-fA-F]+)u", hdr)
    assert m and int(m.group(1), 16) == rl_amd.TALLY_ACCUMULATE == 1
    assert (rl_amd.TALLY_ROWS, rl_amd.TALLY_UNKNOWN) == (256, 255)
    m = re.search(r"#define RL_MAX_LIMITERS\s+(\d+)", hdr)
    assert int(m.group(1)) == rl_amd.TALLY_UNKNOWN            # ids are 0..254: row 255 is free
    assert ctypes.sizeof(rl_amd.LimiterTally) == 96 == rl_amd.TALLY_DTYPE.itemsize
    body = re.search(r"typedef struct rl_limiter_tally \{(.*?)\} rl_limiter_tally;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f for decl in re.findall(r"uint64_t\s+([^;]+);", body) for f in re.findall(r"[a-z_]+", decl)]
    assert fields == [f for f, _ in rl_amd.LimiterTally._fields_] == list(rl_amd.TALLY_DTYPE.names)


def test_invalid_arguments_are_rejected_before_any_device_call():
    """A null engine is checked first, so every listed case runs without a GPU and leaves the
    outputs holding their fill pattern."""
    L = rl_amd.lib()
    bad = rl_amd.RL_E_INVALID_ARG
    p = rl_amd._p
    permits = np.array([1, 1, 1], np.int32)
    lim = np.zeros(3, np.uint16)
    op = np.zeros(3, np.uint8)
    al = np.array([1, 0, 0], np.uint8)
    rem = np.array([2, 0, 0], np.int64)
    keys = np.array([1, 2, 2], np.uint64)
    out = np.zeros(rl_amd.TALLY_ROWS, rl_amd.TALLY_DTYPE)
    out.view(np.uint8)[:] = 0x5A
    before = out.tobytes()
    odd = ctypes.c_void_p(out.ctypes.data + 4)                 # not 8-byte aligned

    def tally(e, n, pp, aa, rr, oo, flags):
        return (L.rl_tally_batch(e, n, pp, p(lim), p(op), aa, rr, oo, flags),
                L.rl_tally_batch_device(e, n, pp, p(lim), p(op), aa, rr, oo, flags, None))

    for args in ((3, p(permits), p(al), p(rem), p(out), 0),            # only the engine is missing
                 (3, None, p(al), p(rem), p(out), 0),
                 (3, p(permits), None, p(rem), p(out), 0),
                 (3, p(permits), p(al), None, p(out), 0),
                 (3, p(permits), p(al), p(rem), None, 0),
                 (0, None, None, None, None, 0),
                 (3, p(permits), p(al), p(rem), p(out), 2),            # unknown flag bits
                 (3, p(permits), p(al), p(rem), p(out), 0x80000001),
                 (3, p(permits), p(al), p(rem), odd, 0),
                 ((1 << 31) + 1, p(permits), p(al), p(rem), p(out), 0)):
        assert tally(None, *args) == (bad, bad), args
    assert L.rl_tally_batch(None, 3, p(permits), None, None, p(al), p(rem), p(out), 1) == bad
    assert out.tobytes() == before

    top = np.full(4, 7, np.uint64)
    cnt = np.full(4, 7, np.uint64)
    hdr = np.full(4, 7, np.uint64)
    n_out = ctypes.c_size_t(7)
    heavy, denied = ctypes.c_uint64(7), ctypes.c_uint64(7)

    def host(e, n, kk, pp, aa, rr, sel, k, mc, t=top, c=cnt, no=ctypes.byref(n_out), nh=ctypes.byref(heavy)):
        return L.rl_top_denied(e, n, kk, pp, p(lim), p(op), aa, rr, sel, k, mc, p(t), p(c), no, nh,
                               ctypes.byref(denied))

    def dev(e, n, kk, pp, aa, rr, sel, k, mc, t=top, c=cnt, h=hdr):
        return L.rl_top_denied_device(e, n, kk, pp, p(lim), p(op), aa, rr, sel, k, mc, p(t), p(c), p(h), None)

    ok = (3, p(keys), p(permits), p(al), p(rem))
    for sel, k, mc in ((0, 4, 1), (300, 4, 1), (0, 0, 1), (0, 4097, 1), (0, 4, 0)):
        assert host(None, *ok, sel, k, mc) == bad and dev(None, *ok, sel, k, mc) == bad
    for i in range(1, 5):                                              # each array missing in turn
        args = list(ok)
        args[i] = None
        assert host(None, *args, 0, 4, 1) == bad and dev(None, *args, 0, 4, 1) == bad
    assert host(None, *ok, 0, 4, 1, t=None) == bad and dev(None, *ok, 0, 4, 1, t=None) == bad
    assert host(None, *ok, 0, 4, 1, c=None) == bad and dev(None, *ok, 0, 4, 1, c=None) == bad
    assert host(None, *ok, 0, 4, 1, no=None) == bad and host(None, *ok, 0, 4, 1, nh=None) == bad
    assert dev(None, *ok, 0, 4, 1, h=None) == bad
    assert host(None, (1 << 31) + 1, *ok[1:], 0, 4, 1) == bad
    assert np.all(top == 7) and np.all(cnt == 7) and np.all(hdr == 7)
    assert (n_out.value, heavy.value, denied.value) == (7, 7, 7)
