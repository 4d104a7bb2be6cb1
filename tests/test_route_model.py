"""tests/route_model.py, the reference of the routing kernels, checked on the CPU: every fold /
unfold pair is the identity on its documented domain; the model agrees byte for byte with
test_router_gloo.HostOps (the stand-in the Python router runs on) on that test's own trace, so
that there are not two definitions drifting apart; a layout of G segments is G one-segment
layouts in a row; and every input set of tests/test_gpu_route_kernels.py (tests/route_cases.py)
has the properties that test relies on."""
import numpy as np
import pytest
import torch

import rl_amd
import route_cases as rc
import route_model as rm
from oracle.coracle import COracle
from rl_amd.router import EXC_CAP
from test_router_gloo import LIMS, HostOps, global_trace


# ---------------------------------------------------------------- identities
def test_fold_is_the_identity():
    for n in rc.SIZES:
        a, r = rc.fold_case(n)
        p = rm.fold(a, r)
        assert np.array_equal(p, r * 2 + (a & 1))
        a2, r2 = rm.unfold(p)
        assert np.array_equal(a2, a & 1) and np.array_equal(r2, r)
    a, r = rc.fold_case(5000)
    assert set(r.tolist()) == set(rc.FOLD_REMAINING) and set(a.tolist()) == set(rc.FOLD_ALLOWED)


def test_width_hi():
    assert [rm.width_hi(w) for w in rc.WIDTHS] == [124, 32764, 2 ** 31 - 4, 2 ** 63 - 4]


@pytest.mark.parametrize("w", rc.WIDTHS)
def test_fold_packed_is_the_identity_on_its_domain(w):
    hi = rm.width_hi(w)
    for n in rc.SIZES:
        a, r = rc.packed_case(n, w)
        assert np.all((r >= -3) & (r <= hi)) and not np.any((a & 1 == 1) & (r == -3))
        if n >= 256:                                # both ends and the sentinels are there
            assert {-3, -2, -1, hi} <= set(r.tolist())
            assert {0, 1, 0xFF} == set(a.tolist())
        b = rm.fold_packed(a, r, w)
        assert b.dtype == np.uint8 and b.size == n * w
        assert not np.any(b.view(rm._U[w]) == rm.ESCAPE)
        a2, r2 = rm.unfold_packed(b, w)
        assert np.array_equal(a2, a & 1) and np.array_equal(r2, r)
    # little-endian words of (remaining + 3) << 1 | allowed
    assert rm.fold_packed([1], [0], w).tolist() == [7] + [0] * (w - 1)
    assert rm.fold_packed([0], [hi], w).tolist() == [0xFE] + [0xFF] * (w - 1)


def test_ops_column_is_the_identity_below_the_clamps():
    perm, lim, op = rc.ops_case(5000)
    col = rm.fold_ops(perm, lim, op)
    l2, o2 = rm.unfold_ops(col)
    assert np.array_equal(l2, np.minimum(lim[perm], 0x3FFF)) and np.array_equal(o2, np.minimum(op[perm], 3))
    assert np.all(l2[lim[perm] > 255] > 255) and np.all(o2[op[perm] > 2] == 3)
    assert np.array_equal(rm.fold_ops(perm, None, None), np.zeros(5000, np.uint16))


def test_wire_is_the_identity_inside_its_window():
    for epoch in rc.WIRE_EPOCHS:
        perm, keys, permits, now, _ = rc.wire_case(257, epoch)
        wire, base, ovf = rm.pack_wire(perm, keys, permits, now)
        assert ovf == 0 and base == np.floor_divide(now[0], rc.NS) - 2 ** 31
        k, p, t = rm.unwire(wire, [base], [257])
        assert np.array_equal(k, keys[perm]) and np.array_equal(p, permits[perm])
        assert np.array_equal(t, np.floor_divide(now[perm], rc.NS) * rc.NS)
    assert rm.pack_wire(np.zeros(0, np.uint32), [], [], [])[1:] == (0, 0)


# ---------------------------------------------------------------- the model against HostOps
W, N, STEPS = 4, 3000, 2


def _slices(regress=False, span_ms=20_000):
    keys, permits, now, lim = global_trace(STEPS, W, N, span_ms, regress)
    for s in range(STEPS * W):
        sl = slice(s * N, (s + 1) * N)
        yield keys[sl], permits[sl], now[sl], lim[sl]


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype).copy())


def test_partition_pack_and_wire_agree_with_hostops():
    ops = HostOps(W)
    for span in (20_000, 1 << 36):
        for keys, permits, now, lim in _slices(span_ms=span):
            hdr = ops.header()
            ops.partition(N, _t(keys, np.int64), hdr)
            perm, counts = rm.partition(rm.owners(keys, W), None, W)
            assert np.array_equal(ops.perm, perm) and np.array_equal(hdr[:, 0].numpy(), counts)
            k, p, t, l = ops.pack(N, _t(keys, np.int64), _t(permits, np.int32), _t(now, np.int64),
                                  _t(lim, np.int16))
            mk, mp_, mt, ml = rm.pack(perm, keys, permits, now, lim)
            assert np.array_equal(k.numpy().view(np.uint64), mk) and np.array_equal(p.numpy(), mp_)
            assert np.array_equal(t.numpy(), mt) and np.array_equal(l.numpy().view(np.uint16), ml)
            wire, wl, whdr = ops.pack_wire(N, _t(keys, np.int64), _t(permits, np.int32),
                                           _t(now, np.int64), _t(lim, np.int16))
            mw, base, ovf = rm.pack_wire(perm, keys, permits, now)
            assert wire.numpy().tobytes() == mw.tobytes()
            assert whdr.tolist() == [base, ovf] and ovf == (span > 1 << 32)
            assert np.array_equal(wl.numpy().view(np.uint16), ml)
            if not ovf:
                bases, cnts = [base, base - 5, base + 7], [1000, 0, 2000]
                hk, hp, ht = ops.unwire(N, wire, bases, cnts)
                uk, up, ut = rm.unwire(mw, bases, cnts)
                assert np.array_equal(hk.numpy().view(np.uint64), uk)
                assert np.array_equal(hp.numpy(), up) and np.array_equal(ht.numpy(), ut)


def test_fold_agrees_with_hostops():
    ops, orc = HostOps(W), COracle(LIMS)
    for keys, permits, now, lim in _slices(regress=True):
        a, r, _, _ = orc.run(keys, permits, now, lim, None, want_tokens=False)
        back = ops.decide(N, _t(keys, np.int64), _t(permits, np.int32), _t(now, np.int64), _t(lim, np.int16))
        assert np.array_equal(back.numpy(), rm.fold(a, r))
        ops.perm = np.random.default_rng(1).permutation(N)
        ha, hr = torch.zeros(N, dtype=torch.uint8), torch.zeros(N, dtype=torch.int64)
        ops.unpack(N, back, ha, hr)
        ma, mr = rm.scatter(ops.perm, N, *rm.unfold(back.numpy()))
        assert np.array_equal(ha.numpy(), ma) and np.array_equal(hr.numpy(), mr)
        assert np.array_equal(ma[ops.perm], a) and np.array_equal(mr[ops.perm], r)


@pytest.mark.parametrize("w", rc.WIDTHS)
def test_return_trip_agrees_with_hostops(w):
    ops, orc = HostOps(W), COracle(LIMS)
    counts = [700, 0, 1801, 499]
    escapes = 0
    for keys, permits, now, lim in _slices(regress=True):
        a, r, _, _ = orc.run(keys, permits, now, lim, None, want_tokens=False)
        out = ops.decide_return(N, _t(keys, np.int64), _t(permits, np.int32), _t(now, np.int64),
                                _t(lim, np.int16), w, counts).numpy()
        want = rm.fold_return_buffer(a, r, counts, w, EXC_CAP)
        assert out.tobytes() == want.tobytes()
        assert ops.return_bytes(counts, w) == rm.return_bytes(counts, w, EXC_CAP) == want.size
        escapes += int((~rm.fits(r, w)).sum())
        # the buffer as it is, and with segment 2's block emptied: its escapes are lost
        cut = out.copy()
        cut[rm.ret_layout(counts, w, EXC_CAP)[1][2]:][:8] = 0
        for buf in (out, cut):
            ops.perm = np.random.default_rng(w).permutation(N)
            ops._lost = 0
            ha, hr = torch.zeros(N, dtype=torch.uint8), torch.zeros(N, dtype=torch.int64)
            ops.unpack_return(N, torch.from_numpy(buf), w, counts, ha, hr)
            ma, mr, lost = rm.unpack_return(buf, counts, w, EXC_CAP, ops.perm)
            assert np.array_equal(ha.numpy(), ma) and np.array_equal(hr.numpy(), mr)
            assert ops.lost() == lost
        seg2 = slice(700, 2501)
        assert lost == int((~rm.fits(r[seg2], w)).sum())
    assert ops.escapes == escapes
    if w == 1:
        assert escapes > 50


# ---------------------------------------------------------------- layouts
@pytest.mark.parametrize("w", rc.WIDTHS)
@pytest.mark.parametrize("cap", rc.EXC_CAPS)
def test_layout_of_segments_is_one_segment_layouts_in_a_row(w, cap):
    for name, counts in rc.SEG_LISTS.items():
        seg, blk, tot = rm.ret_layout(counts, w, cap)
        o = 0
        for s, c in enumerate(counts):
            s1, b1, t1 = rm.ret_layout([c], w, cap)
            assert (seg[s], blk[s]) == (o + s1[0], o + b1[0]), (name, s)
            assert b1[0] % 8 == 0 and 0 <= b1[0] - c * w < 8 and t1 == b1[0] + 8 + 16 * cap
            o += t1
        assert tot == o == sum(rm.return_bytes([c], w, cap) for c in counts)
    assert rm.return_bytes([], w, cap) == 0 and rm.return_bytes([1] * 65, w, cap) == 0
    assert rm.return_bytes([1], 3, cap) == 0


# ---------------------------------------------------------------- the GPU tests' inputs
@pytest.mark.parametrize("shards", rc.PART_SHARDS)
def test_adversarial_owner_patterns_are_what_they_claim(shards):
    assert all(p.size >= 64 for p in rc.owner_pools(shards))
    lanes = np.arange(rc.PART_N) % 64
    for pattern in rc.PATTERNS:
        keys = rc.pattern_keys(pattern, shards)
        own = rm.owners(keys, shards)
        assert keys.size == rc.PART_N == 2 * rc.TILE + 777
        assert np.array_equal(own, rc.pattern_owners(pattern, shards)), pattern
        counts = np.bincount(own, minlength=shards)
        if pattern == "one":
            assert (counts > 0).sum() == 1
        elif pattern == "round_robin":              # a wave holds 64 / shards requests of every owner
            full = own[:rc.PART_N // 64 * 64].reshape(-1, 64)
            assert all(np.array_equal(np.bincount(row, minlength=shards), np.full(shards, 64 // shards))
                       for row in full[:: 97])
            if shards == 64:
                assert np.all(np.sort(full, 1) == np.arange(64))
        elif pattern == "runs":                     # owners change inside a wave, at lane 37
            sw = np.nonzero(own[1:] != own[:-1])[0] + 1
            assert sw.size > 2000 and np.all(lanes[sw] == rc.RUN_SWITCH)
        elif pattern == "descending":
            assert np.all(np.diff(own.astype(np.int64)) <= 0) and np.all(counts > 0)
        elif pattern == "absent":
            assert counts[0] == 0 and np.all(counts[1:] > 0)
        skip = rc.skip_mask(pattern, shards)
        assert 0.45 < (skip != 0).mean() < 0.55 and len(set(skip.tolist())) > 100
        perm, c = rm.partition(own, skip, shards)
        assert c.sum() == perm.size == (skip == 0).sum()
        assert np.all(np.diff(own[perm].astype(np.int64)) >= 0)


def test_full_directory_case():
    dk, do = rc.full_directory()
    assert dk.size == 4096 == len(set(dk.tolist())) and do.max() == 63 and do.min() == 0
    assert np.array_equal(do, (3 + 7 * np.arange(4096)) % 64)
    moved = do != rm.owners(dk, 64)
    assert moved.mean() > 0.9                        # the directory, not the hash, decides
    keys, hit = rc.directory_batch()
    assert keys.size == 70_000 and hit.sum() == 35_000
    assert np.all(np.isin(keys[hit], dk)) and not np.any(np.isin(keys[~hit], dk))
    own = rm.owners(keys, 64, dk, do)
    look = dict(zip(dk.tolist(), do.tolist()))
    assert own[hit].tolist() == [look[k] for k in keys[hit].tolist()]
    assert np.array_equal(own[~hit], rl_amd.owner_of(keys[~hit], 64))
    assert not np.any(np.isin(rc.other_keys(), dk))
    assert rc.full_directory(4097)[0].size == 4097


@pytest.mark.parametrize("w", rc.WIDTHS)
@pytest.mark.parametrize("cap", rc.EXC_CAPS)
def test_return_cases_hold_the_stated_escapes(w, cap):
    hi = rm.width_hi(w)
    first = last = over = exact = 0
    for name, counts in rc.SEG_LISTS.items():
        assert {(c * w) % 8 for c in rc.SEG_LISTS["residues"]} == set(range(0, 8, np.gcd(w, 8)))
        for kind in rc.ESC_KINDS:
            got, a, r, perm = rc.return_case(name, w, cap, kind)
            assert got == counts and a.size == r.size == perm.size == sum(counts)
            assert np.array_equal(np.sort(perm), np.arange(sum(counts)))
            esc = ~rm.fits(r, w)
            assert np.all((r[esc] < -3) | ((r[esc] > hi) & (a[esc] & 1 == 0)))
            assert not np.any(~esc & (a & 1 == 1) & (r == -3))          # no stray escape code
            want = rc.escape_targets(counts, cap, kind)
            folded = rm.fold_return(a, r, counts, w)
            beg = 0
            for s, c in enumerate(counts):
                e = esc[beg:beg + c]
                assert int(e.sum()) == want[s] == len(folded[s][1]), (name, kind, s)
                assert np.array_equal(np.nonzero(folded[s][0].view(rm._U[w]) == rm.ESCAPE)[0], np.nonzero(e)[0])
                if c:
                    first += bool(e[0])
                    last += bool(e[-1])
                over += want[s] > cap
                exact += want[s] == cap and cap > 0
                beg += c
            if name == "one":
                base = {"none": 0, "cap": cap, "cap_plus_1": cap + 1, "cap_plus_5": cap + 5}[kind]
                assert want == [base]                                    # RET_N holds every target
            if w < 8 and kind != "none" and sum(want) > 20:
                assert np.any(r[esc] > hi) and np.any(r[esc] < -3)
    assert first and last and over and (exact or cap == 0)
    assert [len(c) for c in rc.SEG_LISTS.values()] == [1, 2, 2, 5, 64, 8]
    assert rc.SEG_LISTS["sixty_four"].count(0) >= 5 and rc.SEG_LISTS["small"] == [3, 0, 0, 5, 1]


def test_wire_cases():
    assert rc.WIRE_BIG == 2048 * 256 + 321
    for epoch, t0 in rc.WIRE_EPOCHS.items():
        for n in rc.WIRE_SIZES[1:3]:
            perm, keys, permits, now, lim = rc.wire_case(n, epoch)
            assert now[0] == t0 and np.all(now % rc.NS != 0)
            assert rm.pack_wire(perm, keys, permits, now)[2] == 0
            assert np.any(permits < 0) or n == 1
        _, _, _, now, _ = rc.wire_case(257, epoch)
        assert (epoch == "epoch") == bool(np.any(now < 0)) and (epoch != "epoch" or np.any(now > 0))
        for off, flag in rc.WIRE_EDGES:
            for n, last in ((257, False), (rc.WIRE_BIG, True)):
                perm, keys, permits, now, lim, j = rc.wire_edge_case(n, epoch, off, last)
                assert perm[j] != 0 and (j >= rc.WIRE_BLOCKS_MAX * 256) == last
                ms = np.floor_divide(now, rc.NS)
                assert ms[perm[j]] - ms[0] == off
                wire, base, ovf = rm.pack_wire(perm, keys, permits, now)
                assert ovf == flag and base == ms[0] - 2 ** 31
                out = (ms - base < 0) | (ms - base > 0xFFFFFFFF)
                assert out.sum() == flag and (not flag or out[perm[j]])
    assert len(set(rc.UNWIRE_BASES)) == 64 and min(rc.UNWIRE_BASES) < 0 < max(rc.UNWIRE_BASES)
    assert rc.UNWIRE_COUNTS.count(0) >= 5 and rc.unwire_case().shape == (sum(rc.UNWIRE_COUNTS), 2)
