"""CPU-side checks of rl_key_hash and of rl_hash_keys / rl_hash_keys_device / rl_execute_batch_keys
at the C-ABI boundary (no device calls)."""
import ctypes
import re

import numpy as np

import rl_amd

NEW = ["rl_key_hash", "rl_hash_keys", "rl_hash_keys_device", "rl_execute_batch_keys"]

# computed with a Python restatement of ratelimiter::keyHash as it was before rl_key_hash
KNOWN = [(b"", 0xF52A15E9A9B5E89B), (b"a", 0x02C0BDBF481420F8), (b"user:42", 0xD68CB863FC5E0C34),
         (b"anonymous", 0x730735840277EA9A), (b"\x00", 0x25FC6DD36CE04B20),
         (b"\xff\x00\x80", 0x386053F1EFB4A7F5),
         ("clé-€".encode("utf-8"), 0x998D7A6DD3954E86)]


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


def test_the_header_states_the_length_limit_and_the_formula():
    hdr = open(rl_amd.HEADER).read()
    m = re.search(r"#define RL_KEY_MAX_BYTES\s+(\d+)\b", hdr)
    assert m and int(m.group(1)) == 4096 == rl_amd.KEY_MAX_BYTES
    flat = " ".join(hdr.split()).replace(" * ", " ")           # (comment continuation stars)
    for piece in ("h = 0xcbf29ce484222325;", "h = (h ^ c) * 0x100000001b3;", "rl_key_hash = mix64(h)",
                  "0xbf58476d1ce4e5b9", "0x94d049bb133111eb", "UNSIGNED"):
        assert piece.replace(" * ", " ") in flat, piece


def test_known_answers():
    assert KNOWN[6][0] == bytes.fromhex("636cc3a92de282ac")
    for b, want in KNOWN:
        assert rl_amd.key_hash(b) == want, b
        assert rl_amd.key_hash_model(b) == want, b
    assert rl_amd.key_hash("clé-€") == KNOWN[6][1]      # a str is its UTF-8 bytes
    assert rl_amd.lib().rl_key_hash(None, 0) == KNOWN[0][1]       # NULL with len 0


def test_the_host_hash_equals_the_model_on_random_bytes():
    """Lengths 0..300 with 0x00 and bytes >= 0x80 among them: a signed-char or a C-string bug
    shows here."""
    rng = np.random.default_rng(20240607)
    seen_zero = seen_high = 0
    for i in range(2000):
        b = rng.integers(0, 256, int(rng.integers(0, 301)), dtype=np.uint8).tobytes()
        if i % 7 == 0:
            b = b[:len(b) // 2] + b"\x00\xff\x80" + b[len(b) // 2:]
        seen_zero += 0 in b
        seen_high += any(c >= 0x80 for c in b)
        assert rl_amd.key_hash(b) == rl_amd.key_hash_model(b), b.hex()
    assert seen_zero > 500 and seen_high > 1500


def test_pack_keys_layout():
    blob, off = rl_amd.pack_keys([b"ab", b"", "cé"], first_offset=3)
    assert off.dtype == np.uint64 and off.tolist() == [3, 5, 5, 8]
    assert blob.dtype == np.uint8 and blob[3:].tobytes() == b"abc\xc3\xa9" and blob.shape[0] == 8
    blob, off = rl_amd.pack_keys([])
    assert off.tolist() == [0] and blob.shape[0] == 0


def test_invalid_arguments_are_rejected_before_any_device_call():
    """A null engine is checked first, so every case runs without a GPU, and every output byte
    stays untouched."""
    L = rl_amd.lib()
    bad = rl_amd.RL_E_INVALID_ARG
    blob, off = rl_amd.pack_keys([b"user:42", b"", b"anonymous"])
    n = 3
    outs = {"hash": np.zeros(n, np.uint64), "hdr": np.zeros(2, np.uint64), "allowed": np.zeros(n, np.uint8),
            "remaining": np.zeros(n, np.int64), "tokens": np.zeros(n, np.float64)}
    for a in outs.values():
        a.view(np.uint8)[:] = 0x5A
    before = {k: a.tobytes() for k, a in outs.items()}
    permits, now = np.ones(n, np.int32), np.zeros(n, np.int64)
    p = rl_amd._p
    for nn, bl in ((n, len(blob)), (0, 0), (n, 2), (1 << 40, len(blob))):
        assert L.rl_hash_keys(None, nn, p(blob), bl, p(off), p(outs["hash"])) == bad
        assert L.rl_hash_keys_device(None, nn, p(blob), bl, p(off), p(outs["hash"]), p(outs["hdr"]), None) == bad
        assert L.rl_execute_batch_keys(None, nn, p(blob), bl, p(off), p(permits), p(now), None, None,
                                       p(outs["allowed"]), p(outs["remaining"]), p(outs["tokens"]),
                                       p(outs["hash"])) == bad
    assert L.rl_hash_keys(None, n, None, 0, None, None) == bad
    assert L.rl_hash_keys_device(None, n, None, 0, None, None, None, None) == bad
    for k, a in outs.items():
        assert a.tobytes() == before[k], k
