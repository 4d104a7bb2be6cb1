"""CPU-side checks of rl_limiter_digest / rl_limiter_digest_device at the C-ABI boundary (no device calls)."""
import ctypes
import re

import numpy as np

import rl_amd

NEW = ["rl_limiter_digest", "rl_limiter_digest_device"]


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


def test_the_struct_is_24_bytes_with_the_headers_fields():
    hdr = open(rl_amd.HEADER).read()
    assert ctypes.sizeof(rl_amd.BucketDigest) == 24 == rl_amd.DIGEST_DTYPE.itemsize
    body = re.search(r"typedef struct rl_bucket_digest \{(.*?)\} rl_bucket_digest;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"uint64_t\s+(\w+)", body)
    assert fields == [f for f, _ in rl_amd.BucketDigest._fields_] == list(rl_amd.DIGEST_DTYPE.names)
    m = re.search(r"#define RL_DIGEST_CACHE\s+0x([0-9a-fA-F]+)u", hdr)
    assert m and int(m.group(1), 16) == rl_amd.DIGEST_CACHE == 1


def test_the_header_states_the_constants_and_the_formula_of_the_model():
    hdr = open(rl_amd.HEADER).read()
    for name, val in (("RL_DIGEST_K_SW", rl_amd.DIGEST_K[0]), ("RL_DIGEST_K_TB", rl_amd.DIGEST_K[1]),
                      ("RL_DIGEST_K_CACHE", rl_amd.DIGEST_K[2]), ("RL_DIGEST_C1", rl_amd.DIGEST_C1),
                      ("RL_DIGEST_C2", rl_amd.DIGEST_C2)):
        m = re.search(rf"#define {name}\s+0x([0-9a-fA-F]{{16}})ULL", hdr)
        assert m, name
        assert int(m.group(1), 16) == val, name
        assert val & 1, name                                   # odd: the multiplies are bijections
    assert len({*rl_amd.DIGEST_K, rl_amd.DIGEST_C1, rl_amd.DIGEST_C2}) == 5
    flat = " ".join(hdr.split()).replace(" * ", " ")           # (comment continuation stars)
    for piece in ("u = tag + K[kind];", "u = (u ^ f1) * C1;", "u = (u ^ rotl(f2, 23)) * C2;",
                  "u ^= rotl(f3, 47);", "H = mix64(u)", "0xbf58476d1ce4e5b9", "0x94d049bb133111eb",
                  "What equality means"):
        assert piece.replace(" * ", " ") in flat, piece


def test_invalid_arguments_are_rejected_before_any_device_call():
    """A null engine is checked first, so every case runs without a GPU, and `out` and `total`
    stay untouched."""
    L = rl_amd.lib()
    bad = rl_amd.RL_E_INVALID_ARG
    out = np.zeros(8, rl_amd.DIGEST_DTYPE)
    out.view(np.uint8)[:] = 0x5A
    before = out.tobytes()
    tot = rl_amd.BucketDigest()
    ctypes.memset(ctypes.byref(tot), 0x5A, ctypes.sizeof(tot))
    tot_before = bytes(tot)
    for lim, bits, flags in ((0, 0, 0), (9, 3, 1), (0, 3, 2), (0, 99, 0)):
        assert L.rl_limiter_digest(None, lim, 0, bits, flags, rl_amd._p(out), ctypes.byref(tot)) == bad
        assert L.rl_limiter_digest(None, lim, 0, bits, flags, rl_amd._p(out), None) == bad
        assert L.rl_limiter_digest_device(None, lim, 0, bits, flags, rl_amd._p(out), None) == bad
    assert L.rl_limiter_digest(None, 0, 0, 0, 0, None, ctypes.byref(tot)) == bad
    assert L.rl_limiter_digest_device(None, 0, 0, 0, 0, None, None) == bad
    assert out.tobytes() == before and bytes(tot) == tot_before
