"""Every routing kernel behind the multi-GPU router, one by one on the GPU, held to the numpy
reference tests/route_model.py: the owner partition at the shard counts the header promises
(adversarial owner patterns, a full directory), rl_route_pack, the int64 and the packed folds,
the segmented return trip (segments, padding, exception blocks, `lost`), the compact wire past
one grid stride and on both sides of its window, and the ops column. Inputs come from
tests/route_cases.py (their properties are asserted on the CPU by tests/test_route_model.py).
Every output is pre-filled with a sentinel byte and followed by a guard that must come back
untouched; bytes and whole arrays are compared with np.array_equal."""
import numpy as np
import pytest
import torch

import rl_amd
import route_cases as rc
import route_model as rm

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT64 = np.frombuffer(bytes([rc.SENT]) * 8, np.int64)[0]
_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}


def _dev(a):
    """numpy -> device tensor of the same bytes, never empty (an empty batch still hands the
    entry points real pointers). The copy is complete when this returns."""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype)).copy()).to(DEV)


def _out(nbytes):
    """An output of nbytes and its guard, all sentinel bytes (uploaded, not filled by a kernel
    on another stream than the engine's)."""
    return torch.from_numpy(np.full(nbytes + rc.GUARD, rc.SENT, np.uint8)).to(DEV)


def _get(t, nbytes, dtype=np.uint8):
    """The output's bytes after a device-wide synchronise; the guard must be intact."""
    torch.cuda.synchronize()
    b = t.cpu().numpy()
    assert b.size == nbytes + rc.GUARD and np.all(b[nbytes:] == rc.SENT), "guard overwritten"
    return b[:nbytes].view(dtype)


def _untouched(t, nbytes):
    return bool(np.all(_get(t, nbytes) == rc.SENT))


def _invalid(call, *args):
    with pytest.raises(rl_amd.RlError) as ei:
        call(*args)
    assert ei.value.status == rl_amd.RL_E_INVALID_ARG


_engines = {}


def _engine(shards):
    """One engine per shard count; a test that needs a directory installs (or clears) it itself."""
    if shards not in _engines:
        e = rl_amd.Engine(device=0, max_batch=1 << 12, capacity=1 << 10, shard_index=0, shard_count=shards)
        e.add_limiter(rl_amd.TB, 50, 60_000, 10.0)
        _engines[shards] = e
    return _engines[shards]


# ---------------------------------------------------------------- owner partition
STRIDE = 3                                           # the counts land STRIDE int64 apart


def _check_partition(eng, keys, own, skip, shards, host_counts):
    """rl_route_partition_skip_device against the model; with a NULL mask also
    rl_route_partition_device and (host_counts) rl_route_partition."""
    n = keys.size
    want, cnt = rm.partition(own, skip, shards)
    kd = _dev(keys)
    sd = None if skip is None else _dev(skip)
    perm, counts = _out(4 * n), _out(8 * shards * STRIDE)
    eng.route_partition_skip_device(n, kd, sd, perm, shards, counts, STRIDE)
    got = _get(perm, 4 * n, np.uint32)
    c = _get(counts, 8 * shards * STRIDE, np.int64).reshape(shards, STRIDE)
    assert np.array_equal(c[:, 0], cnt) and np.all(c[:, 1:] == SENT64)
    assert np.array_equal(got[:want.size], want)
    assert np.all(got[want.size:].view(np.uint8) == rc.SENT)           # the tail is not written
    if skip is None:
        perm2, counts2 = _out(4 * n), _out(8 * shards * STRIDE)
        eng.route_partition_device(n, kd, perm2, shards, counts2, STRIDE)
        assert np.array_equal(_get(perm2, 4 * n, np.uint32), got)
        assert np.array_equal(_get(counts2, 8 * shards * STRIDE, np.int64).reshape(shards, STRIDE), c)
        if host_counts:
            perm3 = _out(4 * n)
            hc = eng.route_partition(n, kd, perm3, shards)
            assert np.array_equal(hc.astype(np.int64), cnt)
            assert np.array_equal(_get(perm3, 4 * n, np.uint32), want)


@pytest.mark.parametrize("shards", rc.PART_SHARDS)
@pytest.mark.parametrize("pattern", rc.PATTERNS)
def test_partition_adversarial_owners(pattern, shards):
    eng = _engine(shards)
    eng.set_owner_directory([], [])
    keys = rc.pattern_keys(pattern, shards)
    own = rm.owners(keys, shards)
    _check_partition(eng, keys, own, None, shards, True)
    _check_partition(eng, keys, own, rc.skip_mask(pattern, shards), shards, False)


@pytest.mark.parametrize("shards", [1, 2, 4, 8, 16, 32, 64])
def test_partition_host_counts_of_an_empty_batch(shards):
    eng = _engine(shards)
    perm = _out(64)
    hc = eng.route_partition(0, _dev(np.zeros(0, np.uint64)), perm, shards)
    assert hc.size == shards and not hc.any() and _untouched(perm, 64)


def test_partition_follows_a_full_directory():
    shards = rc.DIR_SHARDS
    eng = _engine(shards)
    dk, do = rc.full_directory()
    keys, _ = rc.directory_batch()
    own = rm.owners(keys, shards, dk, do)
    others = rc.other_keys()
    try:
        eng.set_owner_directory(dk, do)
        for _ in range(2):
            _check_partition(eng, keys, own, None, shards, True)
            assert [eng.owner_of(k) for k in dk.tolist()] == do.tolist()
            assert [eng.owner_of(k) for k in others.tolist()] == rm.owners(others, shards, dk, do).tolist()
            # a directory that is too long, or names a shard that does not exist, is refused and
            # the installed one stays in force (the second round of this loop)
            big_k, big_o = rc.full_directory(rc.DIR_MAX + 1)
            _invalid(eng.set_owner_directory, big_k, big_o)
            bad = (do + 1).astype(np.uint32)                              # 63 + 1: no such shard
            assert bad.max() == shards
            _invalid(eng.set_owner_directory, dk, bad)
    finally:
        eng.set_owner_directory([], [])
    assert [eng.owner_of(k) for k in dk[:64].tolist()] == rm.owners(dk[:64], shards).tolist()


# ---------------------------------------------------------------- pack, fold, unpack (wide path)
@pytest.mark.parametrize("n", rc.SIZES)
def test_pack(n):
    eng = _engine(1)
    perm, keys, permits, now, lim = rc.request_arrays(n)
    pd, kd, md, td, ld = (_dev(x) for x in (perm, keys, permits, now, lim))
    wk, wp, wt, wl = rm.pack(perm, keys, permits, now, lim)
    for with_lim, with_out in ((True, True), (False, True), (True, False)):
        ko, po, to, lo = _out(8 * n), _out(4 * n), _out(8 * n), _out(2 * n)
        eng.route_pack(n, pd, kd, md, td, ld if with_lim else None, ko, po, to, lo if with_out else None)
        assert np.array_equal(_get(ko, 8 * n, np.uint64), wk)
        assert np.array_equal(_get(po, 4 * n, np.int32), wp)
        assert np.array_equal(_get(to, 8 * n, np.int64), wt)
        if with_out:
            assert np.array_equal(_get(lo, 2 * n, np.uint16), wl if with_lim else rm.pack(perm, None)[0])
        else:
            assert _untouched(lo, 2 * n)


@pytest.mark.parametrize("n", rc.SIZES)
def test_fold_and_unpack(n):
    eng = _engine(1)
    a, r = rc.fold_case(n)
    perm = rc.request_arrays(n)[0]
    packed = _out(8 * n)
    eng.route_fold(n, _dev(a), _dev(r), packed)
    got = _get(packed, 8 * n, np.int64)
    assert np.array_equal(got, rm.fold(a, r))
    ao, ro = _out(n), _out(8 * n)
    eng.route_unpack(n, _dev(perm), packed, ao, ro)
    ga, gr = _get(ao, n), _get(ro, 8 * n, np.int64)
    wa, wr = rm.scatter(perm, n, *rm.unfold(got))
    assert np.array_equal(ga, wa) and np.array_equal(gr, wr)
    assert np.array_equal(ga[perm], a & 1) and np.array_equal(gr[perm], r)


@pytest.mark.parametrize("w", rc.WIDTHS)
@pytest.mark.parametrize("n", rc.SIZES)
def test_fold_packed_and_unpack_packed(n, w):
    """Inside the documented domain only: these two calls have no escape mechanism."""
    eng = _engine(1)
    a, r = rc.packed_case(n, w)
    perm = rc.request_arrays(n)[0]
    packed = _out(w * n)
    eng.route_fold_packed(n, _dev(a), _dev(r), packed, w)
    got = _get(packed, w * n)
    assert np.array_equal(got, rm.fold_packed(a, r, w))
    ao, ro = _out(n), _out(8 * n)
    eng.route_unpack_packed(n, _dev(perm), packed, w, ao, ro)
    ga, gr = _get(ao, n), _get(ro, 8 * n, np.int64)
    wa, wr = rm.scatter(perm, n, *rm.unfold_packed(got, w))
    assert np.array_equal(ga, wa) and np.array_equal(gr, wr)
    assert np.array_equal(ga[perm], a & 1) and np.array_equal(gr[perm], r)
    for bad in (0, 3, 16):
        _invalid(eng.route_fold_packed, n, _dev(a), _dev(r), packed, bad)
        _invalid(eng.route_unpack_packed, n, _dev(perm), packed, bad, ao, ro)


# ---------------------------------------------------------------- segmented return trip
@pytest.mark.parametrize("cap", rc.EXC_CAPS)
@pytest.mark.parametrize("w", rc.WIDTHS)
def test_return_trip(w, cap):
    eng = _engine(1)
    for name in rc.SEG_LISTS:
        for kind in rc.ESC_KINDS:
            counts, a, r, perm = rc.return_case(name, w, cap, kind)
            n, what = sum(counts), (name, w, cap, kind)
            # sizes: the whole layout, and the sum of one-segment calls the router sizes peers with
            total = rm.return_bytes(counts, w, cap)
            assert eng.route_return_bytes(counts, w, cap) == total, what
            assert sum(eng.route_return_bytes([c], w, cap) for c in counts) == total, what
            # fold
            out = _out(total)
            eng.route_fold_return(n, _dev(a), _dev(r), out, w, counts, cap)
            buf = _get(out, total)
            seg, blk, _ = rm.ret_layout(counts, w, cap)
            listed = []
            for s, (data, esc) in enumerate(rm.fold_return(a, r, counts, w)):
                assert np.array_equal(buf[seg[s]:seg[s] + data.size], data), (what, s)    # pads: not compared
                b = buf[blk[s]:blk[s] + 8 + 16 * cap].view(np.int64)
                assert b[0] == len(esc), (what, s)                  # the true count, past cap too
                k = min(len(esc), cap)
                ent = set(zip(b[1:1 + 2 * k:2].tolist(), b[2:2 + 2 * k:2].tolist()))
                assert len(ent) == k and ent <= esc, (what, s)      # distinct escapes, in any order
                assert np.all(b[1 + 2 * k:] == SENT64), (what, s)   # nothing written past them
                listed.append({p for p, _ in ent})
            # unpack, through a random perm, of the buffer the device folded
            ao, ro, lost = _out(n), _out(8 * n), _dev(np.array([7], np.uint32))
            eng.route_unpack_return(n, _dev(perm), out, w, counts, cap, ao, ro, lost)
            ga, gr = _get(ao, n), _get(ro, 8 * n, np.int64)
            ma, mr, mlost = rm.unpack_return(buf, counts, w, cap, perm)
            assert np.array_equal(ga, ma) and np.array_equal(gr, mr), what
            esc = ~rm.fits(r, w)
            isl = np.zeros(n, bool)                                 # escapes that a block lists
            for beg, ps in zip(np.cumsum([0] + counts[:-1]).tolist(), listed):
                isl[np.array(sorted(ps), np.int64) + beg] = True
            assert not np.any(isl & ~esc), what
            assert np.array_equal(ga[perm], np.where(esc, 0, a & 1)), what
            assert np.array_equal(gr[perm], np.where(esc & ~isl, rm.REMAINING_ERROR, r)), what
            over = sum(max(0, e - cap) for e in rc.escape_targets(counts, cap, kind))
            assert mlost == over == int((esc & ~isl).sum()), what
            assert int(lost.cpu().numpy().view(np.uint32)[0]) == 7 + over, what      # adds to *lost


@pytest.mark.parametrize("w", rc.WIDTHS)
def test_return_trip_argument_errors(w):
    eng = _engine(1)
    cap = 4
    counts, a, r, perm = rc.return_case("small", w, cap, "cap")
    n = sum(counts)
    total = rm.return_bytes(counts, w, cap)
    ad, rd, pd = _dev(a), _dev(r), _dev(perm)
    out, ao, ro, lost = _out(total), _out(n), _out(8 * n), _dev(np.array([7], np.uint32))
    for cnt, width, m in ((counts, w, n + 1), (counts, w, n - 1), ([], w, n), ([0] * 64 + [n], w, n),
                          (counts, 3, n)):
        _invalid(eng.route_fold_return, m, ad, rd, out, width, cnt, cap)
        _invalid(eng.route_unpack_return, m, pd, out, width, cnt, cap, ao, ro, lost)
        assert eng.route_return_bytes(cnt, width, cap) == (total if cnt == counts and width == w else 0)
    assert _untouched(out, total) and _untouched(ao, n) and _untouched(ro, 8 * n)
    assert int(lost.cpu().numpy().view(np.uint32)[0]) == 7


# ---------------------------------------------------------------- compact wire
def _check_wire(eng, perm, keys, permits, now, lim, variants=((True, True), (False, True), (True, False))):
    n = perm.size
    pd, kd, md, td, ld = (_dev(x) for x in (perm, keys, permits, now, lim))
    mw, base, ovf = rm.pack_wire(perm, keys, permits, now)
    for with_lim, with_out in variants:
        wo, lo, hdr = _out(16 * n), _out(2 * n), _out(16)
        eng.route_pack_wire(n, pd, kd, md, td, ld if with_lim else None, wo, lo if with_out else None, hdr)
        assert _get(hdr, 16, np.int64).tolist() == [base, ovf]
        assert np.array_equal(_get(wo, 16 * n, np.uint64).reshape(-1, 2), mw)
        if with_out:
            assert np.array_equal(_get(lo, 2 * n, np.uint16), rm.pack(perm, lim if with_lim else None)[0])
        else:
            assert _untouched(lo, 2 * n)
    return base, ovf


@pytest.mark.parametrize("epoch", list(rc.WIRE_EPOCHS))
@pytest.mark.parametrize("n", rc.WIRE_SIZES)
def test_pack_wire(n, epoch):
    """WIRE_BIG takes a second stride of the capped grid; "epoch" floors negative times."""
    base, ovf = _check_wire(_engine(1), *rc.wire_case(n, epoch))
    assert ovf == 0
    assert base == (0 if n == 0 else np.floor_divide(rc.WIRE_EPOCHS[epoch], rc.NS) - 2 ** 31)


@pytest.mark.parametrize("epoch", list(rc.WIRE_EPOCHS))
@pytest.mark.parametrize("offset_ms,flag", rc.WIRE_EDGES)
def test_pack_wire_overflow_edges(offset_ms, flag, epoch):
    """One request at each edge of [base_ms, base_ms + 2^32), early and late, in the first
    stride of a small batch and in the last stride of a large one."""
    for n, last in ((257, False), (rc.WIRE_BIG, True)):
        perm, keys, permits, now, lim, _ = rc.wire_edge_case(n, epoch, offset_ms, last)
        _, ovf = _check_wire(_engine(1), perm, keys, permits, now, lim, variants=((True, True),))
        assert ovf == flag


def test_unwire_sixty_four_sources():
    eng = _engine(1)
    wire = rc.unwire_case()
    m = wire.shape[0]
    wk, wp, wt = rm.unwire(wire, rc.UNWIRE_BASES, rc.UNWIRE_COUNTS)
    wd = _dev(wire.reshape(-1))
    ko, po, to = _out(8 * m), _out(4 * m), _out(8 * m)
    bad = list(rc.UNWIRE_COUNTS)
    bad[5] += 1
    _invalid(eng.route_unwire, m, wd, rc.UNWIRE_BASES, bad, ko, po, to)
    _invalid(eng.route_unwire, m, wd, rc.UNWIRE_BASES + [0], rc.UNWIRE_COUNTS + [0], ko, po, to)
    assert _untouched(ko, 8 * m) and _untouched(po, 4 * m) and _untouched(to, 8 * m)
    eng.route_unwire(m, wd, rc.UNWIRE_BASES, rc.UNWIRE_COUNTS, ko, po, to)
    assert np.array_equal(_get(ko, 8 * m, np.uint64), wk)
    assert np.array_equal(_get(po, 4 * m, np.int32), wp)
    assert np.array_equal(_get(to, 8 * m, np.int64), wt)
    # one source, and sources that are all empty but one
    for bases, counts in (([-5], [m]), ([1, 2, 3], [0, m, 0])):
        ko, po, to = _out(8 * m), _out(4 * m), _out(8 * m)
        eng.route_unwire(m, wd, bases, counts, ko, po, to)
        assert np.array_equal(_get(to, 8 * m, np.int64), rm.unwire(wire, bases, counts)[2])
        assert np.array_equal(_get(ko, 8 * m, np.uint64), wk) and np.array_equal(_get(po, 4 * m, np.int32), wp)


# ---------------------------------------------------------------- ops column and the wait unpack
@pytest.mark.parametrize("n", rc.SIZES)
def test_ops_column_and_wait(n):
    eng = _engine(1)
    perm, lim, op = rc.ops_case(n)
    pd, ld, od = _dev(perm), _dev(lim), _dev(op)
    for use_lim, use_op in ((True, True), (False, True), (True, False), (False, False)):
        want = rm.fold_ops(perm, lim if use_lim else None, op if use_op else None)
        col = _out(2 * n)
        eng.route_fold_ops(n, pd, ld if use_lim else None, od if use_op else None, col)
        assert np.array_equal(_get(col, 2 * n, np.uint16), want)
        lo, oo = _out(2 * n), _out(n)
        eng.route_unfold_ops(n, col, lo, oo)
        wl, wo = rm.unfold_ops(want)
        assert np.array_equal(_get(lo, 2 * n, np.uint16), wl) and np.array_equal(_get(oo, n), wo)
    back = np.random.default_rng(n).integers(-2, 1 << 40, n).astype(np.int64)
    n_live = n // 2
    skip = np.ones(n, np.uint8)
    skip[perm[:n_live]] = 0
    wait = _out(8 * n)
    eng.route_unpack_wait(n, n_live, pd, _dev(back), _dev(skip), wait)
    assert np.array_equal(_get(wait, 8 * n, np.int64), rm.unpack_wait(n, perm, back, n_live))
