"""rl_hash_keys_device / rl_hash_keys / rl_execute_batch_keys on the GPU. Expected hashes always
come from rl_key_hash on the host (rl_amd.key_hash), never from the kernel."""
import numpy as np
import pytest

import rl_amd

pytestmark = pytest.mark.gpu

U64 = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A
NS = 1_000_000
T0 = 1_700_000_000_000 * NS


def well_formed(o0, o1, bytes_len):
    """The three conditions of include/rl_engine.h."""
    return o0 <= o1 and o1 <= bytes_len and o1 - o0 <= rl_amd.KEY_MAX_BYTES


def host_hashes(blob, off, bytes_len=None):
    """key_hash per key from rl_key_hash on the host; 0 for a malformed key. Returns (hashes,
    malformed count)."""
    bytes_len = blob.shape[0] if bytes_len is None else bytes_len
    raw = blob.tobytes()
    out = np.zeros(off.shape[0] - 1, U64)
    bad = 0
    for i in range(out.shape[0]):
        o0, o1 = int(off[i]), int(off[i + 1])
        if well_formed(o0, o1, bytes_len):
            out[i] = rl_amd.key_hash(raw[o0:o1])
        else:
            bad += 1
    return out, bad


@pytest.fixture(scope="module")
def eng():
    e = rl_amd.Engine(device=0, max_batch=1 << 16, capacity=1 << 12)
    yield e
    e.close()


def device_form(e, blob, off, n=None, bytes_len=None, shift=0, out_len=None):
    """rl_hash_keys_device on copies of the batch in device memory; the blob is placed `shift`
    bytes behind a tensor's base. Returns (the whole output array, hdr)."""
    import torch
    n = off.shape[0] - 1 if n is None else n
    bytes_len = blob.shape[0] if bytes_len is None else bytes_len
    buf = torch.zeros(blob.shape[0] + shift + 16, dtype=torch.uint8, device="cuda")
    if blob.shape[0]:
        buf[shift:shift + blob.shape[0]] = torch.from_numpy(blob).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    out = torch.full((max(n if out_len is None else out_len, 1),), FILL, dtype=torch.int64, device="cuda")
    hdr = torch.full((2,), FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.hash_keys_device(n, buf.data_ptr() + shift, bytes_len, d_off, out, hdr)
    e.sync()
    return out.cpu().numpy().view(U64), hdr.cpu().numpy().view(U64)


def check_device(e, blob, off, **kw):
    want, bad = host_hashes(blob, off, kw.get("bytes_len"))
    got, hdr = device_form(e, blob, off, **kw)
    n = off.shape[0] - 1
    wrong = np.nonzero(got[:n] != want)[0]
    assert wrong.size == 0, (wrong[:8], off[wrong[:8]], off[wrong[:8] + 1])
    assert hdr.tolist() == [bad, n]
    return got


def every_length_at_every_alignment(seed=11):
    """For every start residue r in 0..15 and every length L in 0..80: a filler key that brings
    the running offset to r mod 16, then the key of length L."""
    rng = np.random.default_rng(seed)
    lens = []
    at = 0
    for r in range(16):
        for length in range(81):
            fill = (r - at) % 16
            lens += [fill, length]
            at += fill + length
    off = np.zeros(len(lens) + 1, U64)
    off[1:] = np.cumsum(lens, dtype=U64)
    blob = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    return blob, off


@pytest.fixture(scope="module")
def grid_batch():
    return every_length_at_every_alignment()


def test_every_length_at_every_alignment(eng, grid_batch):
    blob, off = grid_batch
    n = off.shape[0] - 1
    pairs = {(int(off[i + 1] - off[i]), int(off[i]) % 16) for i in range(1, n, 2)}
    assert pairs == {(length, r) for length in range(81) for r in range(16)}     # before any launch
    assert n == 2 * 81 * 16
    assert blob.min() == 0 and blob.max() == 255
    check_device(eng, blob, off)                       # fillers are checked too


@pytest.mark.parametrize("shift", [1, 2, 3, 5, 8, 13])
def test_base_pointer_alignment(eng, grid_batch, shift):
    blob, off = grid_batch
    check_device(eng, blob, off, shift=shift)


def test_length_limit_and_malformed_offsets_beside_good_keys(eng):
    """Lengths 4095, 4096 and 4097, a decreasing offset pair and offsets past key_bytes_len in
    one call. key_bytes_len is passed smaller than the tensor really is, so a wrong read could
    not leave the allocation: the rule is checked without provoking anything."""
    rng = np.random.default_rng(5)
    offs = [7]
    for length in (10, 4095, 4096, 33, 4097, 20):      # key 4 (4097 bytes) is malformed
        offs.append(offs[-1] + length)
    offs.append(offs[-1] - 5)                          # key 6: decreasing
    offs.append(offs[-1] + 30)                         # key 7: fine (overlaps key 5)
    bytes_len = offs[-1] + 64
    offs.append(bytes_len)                             # key 8: ends exactly at key_bytes_len
    offs.append(bytes_len + 1)                         # key 9: one byte past the end
    offs.append(bytes_len + 100)                       # key 10: past the end on both sides
    offs.append(50)                                    # key 11: decreasing, from past the end
    offs.append(90)                                    # key 12: fine
    for length in rng.integers(0, 41, 300):            # and good keys after them
        offs.append(offs[-1] + int(length))
    assert offs[-1] <= bytes_len
    off = np.array(offs, U64)
    blob = rng.integers(0, 256, bytes_len + 8192, dtype=np.uint8)   # the tensor is larger
    want, bad = host_hashes(blob, off, bytes_len)
    assert bad == 5 and [i for i in range(13) if want[i] == 0] == [4, 6, 9, 10, 11]
    got = check_device(eng, blob, off, bytes_len=bytes_len)
    assert (got[[4, 6, 9, 10, 11]] == 0).all()
    # the same with the direct-read path forced
    eng.tune("keys_direct", 1)
    try:
        check_device(eng, blob, off, bytes_len=bytes_len)
    finally:
        eng.tune("keys_direct", 0)


def test_spans_beyond_one_tile_and_tile_transitions(eng):
    rng = np.random.default_rng(6)
    lens = [4096] * 600 + [1] * 1000 + [0] * 1000 + list(rng.integers(1, 41, 300))
    off = np.zeros(len(lens) + 1, U64)
    off[1:] = np.cumsum(lens, dtype=U64)
    blob = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    check_device(eng, blob, off, shift=3)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_ragged_sizes_leave_the_rest_untouched(eng, n):
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 60, 300)
    off = np.zeros(301, U64)
    off[1:] = np.cumsum(lens, dtype=U64)
    blob = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    want, _ = host_hashes(blob, off)
    got, hdr = device_form(eng, blob, off, n=n, out_len=300)
    assert np.array_equal(got[:n], want[:n])
    assert (got[n:] == U64(FILL)).all()
    assert hdr.tolist() == [0, n]


def test_host_form_in_several_chunks():
    rng = np.random.default_rng(7)
    lens = rng.integers(0, 200, 1000)
    lens[rng.integers(0, 1000, 12)] = 4096             # whole-stage keys
    lens[rng.integers(0, 1000, 12)] = 4095
    lens[:3] = (4096, 0, 4096)
    off = np.zeros(1001, U64)
    off[0] = 5
    off[1:] = U64(5) + np.cumsum(lens, dtype=U64)
    blob = rng.integers(0, 256, int(off[-1]) + 9, dtype=np.uint8)
    want, bad = host_hashes(blob, off)
    assert bad == 0
    with rl_amd.Engine(device=0, max_batch=1 << 16, capacity=1 << 12) as one:
        single = one.hash_keys(blob, off)              # one chunk (4 MiB stage, 65,536 keys)
    with rl_amd.Engine(device=0, max_batch=64, capacity=1 << 12) as e:
        e.tune("key_stage_bytes", 4096)
        with pytest.raises(rl_amd.RlError):
            e.tune("key_stage_bytes", 4095)
        chunked = e.hash_keys(blob, off)
        assert np.array_equal(chunked, single)
        assert np.array_equal(chunked, want)
        # a malformed offset: refused on the host, nothing written
        bad_off = off.copy()
        bad_off[500] = bad_off[499] - U64(1) if bad_off[499] else U64(1 << 40)
        out = np.full(1000, FILL, U64)
        st = e._L.rl_hash_keys(e.handle, 1000, rl_amd._p(blob), blob.shape[0], rl_amd._p(bad_off), rl_amd._p(out))
        assert st == rl_amd.RL_E_INVALID_ARG
        assert (out == U64(FILL)).all()
        st = e._L.rl_hash_keys(e.handle, 1000, rl_amd._p(blob), int(off[-1]) - 1, rl_amd._p(off), rl_amd._p(out))
        assert st == rl_amd.RL_E_INVALID_ARG           # the last key ends past key_bytes_len
        assert (out == U64(FILL)).all()
        assert e.hash_keys(*rl_amd.pack_keys([])).shape == (0,)


def _two_limiters(**kw):
    e = rl_amd.Engine(device=0, max_batch=1 << 13, capacity=1 << 12, **kw)
    e.add_limiter(rl_amd.SW, 5, 60_000)
    e.add_limiter(rl_amd.TB, 6, 60_000, refill_per_s=0.5)
    return e


def test_fused_call_equals_execute_batch_on_host_hashes():
    rng = np.random.default_rng(8)
    names = [rng.integers(0, 256, int(length), dtype=np.uint8).tobytes()
             for length in rng.integers(1, 41, 300)]
    assert len(set(names)) == 300
    n = 4096
    with _two_limiters() as a, _two_limiters() as b:
        a.tune("key_stage_bytes", 16384)               # several byte chunks per batch
        for batch in range(3):
            which = rng.integers(0, 300, n)
            blob, off = rl_amd.pack_keys([names[i] for i in which], first_offset=batch)
            hashes = np.array([rl_amd.key_hash(names[i]) for i in which], U64)
            permits = rng.integers(1, 4, n).astype(np.int32)
            permits[rng.integers(0, n, 5)] = 0         # invalid requests: RL_E_INVALID_REQUEST
            now = T0 + (batch * 61_000 + np.sort(rng.integers(0, 600, n))) * NS
            limiter = rng.integers(0, 2, n).astype(np.uint16)
            ga, gr, gt, gst, gh = a.execute_batch_keys(blob, off, permits, now, limiter)
            wa, wr, wt, wst = b.execute(hashes, permits, now, limiter)
            assert gst == wst == rl_amd.RL_E_INVALID_REQUEST
            assert np.array_equal(gh, hashes)
            assert np.array_equal(ga, wa) and np.array_equal(gr, wr)
            assert np.array_equal(gt.view(U64), wt.view(U64))
            assert 0 < int(ga.sum()) < n
            assert a.stats() == b.stats()
            assert a.last_status() == b.last_status() == wst
        # n > max_batch, a malformed offset
        big_blob, big_off = rl_amd.pack_keys([b"k"] * ((1 << 13) + 1))
        z = np.zeros((1 << 13) + 1, np.int64)
        with pytest.raises(rl_amd.RlError) as ei:
            a.execute_batch_keys(big_blob, big_off, z.astype(np.int32), z)
        assert ei.value.status == rl_amd.RL_E_TOO_LARGE
        blob, off = rl_amd.pack_keys([b"abc", b"de"])
        off[1] = 9
        with pytest.raises(rl_amd.RlError) as ei:
            a.execute_batch_keys(blob, off, np.ones(2, np.int32), np.full(2, T0, np.int64))
        assert ei.value.status == rl_amd.RL_E_INVALID_ARG
        assert a.stats() == b.stats()


def test_hash_calls_are_read_only():
    """An rl_hash_keys between two batches changes neither rl_batch_stats_get nor what
    rl_last_status then reports: engine `a` makes the hash calls, its twin `b` does not."""
    import torch
    rng = np.random.default_rng(9)
    n = 2000
    keys = rl_amd.mix64(rng.integers(0, 150, n).astype(U64))
    permits = rng.integers(1, 4, n).astype(np.int32)
    permits[7] = -1                                    # the batch's status: RL_E_INVALID_REQUEST
    limiter = rng.integers(0, 2, n).astype(np.uint16)
    blob, off = rl_amd.pack_keys([b"tenant-%d" % i for i in range(500)])
    want, _ = host_hashes(blob, off)
    outs = []
    with _two_limiters() as a, _two_limiters() as b:
        for e in (a, b):
            now = np.full(n, T0, np.int64)
            d = [torch.from_numpy(x.view(np.int64) if x.dtype == U64 else x).cuda()
                 for x in (keys, permits, now)]
            al = torch.zeros(n, dtype=torch.uint8, device="cuda")
            rem = torch.zeros(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            e.execute_device(n, d[0], d[1], d[2], None, None, al, rem)   # status not collected yet
            if e is a:
                assert np.array_equal(e.hash_keys(blob, off), want)
                got, hdr = device_form(e, blob, off)
                assert np.array_equal(got[:500], want) and hdr.tolist() == [0, 500]
            st = e.last_status()
            outs.append((st, e.stats(), al.cpu().numpy(), rem.cpu().numpy()))
            if e is a:
                assert np.array_equal(e.hash_keys(blob, off), want)
            assert e.last_status() == st and e.stats() == outs[-1][1]
            outs[-1] += e.execute(keys, np.abs(permits), np.full(n, T0 + 5 * NS, np.int64), limiter)[:2]
            outs[-1] += (e.stats(),)
    (sa, sta, ala, rema, a2, r2, st2a), (sb, stb, alb, remb, b2, rb2, st2b) = outs
    assert sa == sb == rl_amd.RL_E_INVALID_REQUEST
    assert sta == stb and st2a == st2b
    assert np.array_equal(ala, alb) and np.array_equal(rema, remb)
    assert np.array_equal(a2, b2) and np.array_equal(r2, rb2)
