"""Every variant of the partition, the local grouping and the unpermute at small shapes,
bit-exact against the CPU oracle (as in test_gpu_parity.py).

The partition tile is shrunk to 8 rounds of 512 requests (rl_tune tile_items=8: 4,096
requests), so a batch of a few thousand requests has full, ragged and several tiles; the
unpermute tile stays 65,536 requests, and the largest batch gives it one full (pipelined)
tile plus a ragged one. Each (knobs, batch size) case runs two batches on a fresh engine, so
that the second one meets state and, on the two-pass table, routes the first one's hot regions.
The traces and the oracle's results are computed once per batch size and shared."""
import functools
import itertools

import numpy as np
import pytest

import rl_amd
from oracle.coracle import COracle
from test_gpu_hot import hot_trace
from test_gpu_parity import NS, T0, assert_same

# sizes of one batch, around the 4,096-request partition tile and the 65,536-request unpermute tile
SIZES = (1, 511, 4095, 4096, 4097, 3 * 4096 + 513, 65536 + 513)
# per size, a seed at which the oracle both allows and denies (checked below on every run)
SEEDS = {1: 9}
LIMS = [[rl_amd.SW, 3, 2_000, 0.0], [rl_amd.TB, 5, 2_000, 1.0]]
BAD_LIMITER = 7


def shape_trace(n, seed):
    """n requests over 3,000 mildly skewed keys of two limiters; about 1 % peeks and resets and
    0.5 % each of unknown limiter ids, unknown operations and zero permits."""
    rng = np.random.default_rng(seed)
    ranks = np.minimum(rng.zipf(1.2, n), 3000) - 1
    keys = rl_amd.mix64(ranks.astype(np.uint64) + np.uint64(seed << 40))
    lim = (ranks % 2).astype(np.uint16)
    now = (T0 * NS + np.sort(rng.integers(0, 4_000 * NS, n))).astype(np.int64)
    permits = rng.integers(1, 3, n).astype(np.int32)
    op = np.zeros(n, np.uint8)
    u = rng.random(n)
    op[u < 0.01] = rl_amd.OP_PEEK
    op[u < 0.005] = rl_amd.OP_RESET
    v = rng.random(n)
    lim[v < 0.005] = BAD_LIMITER
    op[(v >= 0.005) & (v < 0.010)] = 9
    permits[(v >= 0.010) & (v < 0.015)] = 0
    return keys, permits, now, lim, op


@functools.lru_cache(maxsize=None)
def shape_case(n):
    """Two batches of n requests and what the oracle decides (read-only, shared)."""
    tr = shape_trace(2 * n, SEEDS.get(n, 1))
    want = COracle(LIMS).run(*tr)
    for x in tr + want[:3]:
        x.setflags(write=False)
    return tr, want


def check_case_is_meaningful(n, want):
    total = 2 * n
    assert 0 < want[0].sum() < total, f"n={n}: the oracle allows {want[0].sum()} of {total}"
    if n > 1:
        for b in (slice(0, n), slice(n, total)):
            assert 0 < want[0][b].sum() < n, f"n={n}: one batch is all allow or all deny"
    if n >= 4095:
        assert want[3] > 0, f"n={n}: no invalid request"


def run_shapes(capacity, tune, want_tokens):
    """capacity: keys of the whole table, half of them per limiter."""
    for n in SIZES:
        tr, want = shape_case(n)
        check_case_is_meaningful(n, want)
        e = rl_amd.Engine(max_batch=1 << 17, capacity=capacity)
        for l in LIMS:
            e.add_limiter(*l, capacity=capacity // len(LIMS))
        e.tune("tile_items", 8)
        for k, v in tune.items():
            e.tune(k, v)
        got = [[], [], []]
        for b in (slice(0, n), slice(n, 2 * n)):
            a, r, t, st = e.execute(*(x[b] for x in tr), want_tokens=want_tokens)
            assert st in (rl_amd.RL_OK, rl_amd.RL_E_INVALID_REQUEST), rl_amd.strerror(st)
            got[0].append(a); got[1].append(r); got[2].append(t)
        e.close()
        tok = np.concatenate(got[2]) if want_tokens else None
        assert_same((np.concatenate(got[0]), np.concatenate(got[1]), tok), want, f"n={n} {tune}")


# ------------------------------------------------------------------ one-pass table
# 2^14 keys at load 0.5: 2^15 slots, 128 regions, one partition pass. Without balances the
# split unpermute runs where it is asked for; with them k_unpermute's tokens_out path.
ONE_PASS = [dict(scatter_split=ss, wide_records=w, unpermute_split=us)
            for ss, w, us in itertools.product((0, 1), (0, 1), (0, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("tune", ONE_PASS, ids=lambda t: "-".join(f"{k}={v}" for k, v in t.items()))
def test_one_pass_shapes(tune):
    run_shapes(1 << 14, tune, want_tokens=False)


@pytest.mark.gpu
def test_one_pass_shapes_with_balances():
    run_shapes(1 << 14, dict(scatter_split=1, wide_records=0, unpermute_split=1), want_tokens=True)


# ------------------------------------------------------------------ two-pass table
# 2^21 keys at load 0.5: 2^22 slots, 16,384 regions, region ids of 14 bits. group_bits 12: 4,096
# pass-0 bins of 4 regions (s0 = 2), placed by k_gplace_lds; group_bits 3: 8 bins of 2,048
# regions (s0 = 11), placed by k_gplace. hot_threshold 64: the second batch routes the first
# one's hot regions. A pairwise selection: every value of every knob with every value of
# scatter_split and of group_bits (test_two_pass_selection_is_pairwise).
TWO_PASS_KNOBS = dict(scatter_split=(0, 1), wide_records=(0, 1), group_bits=(12, 3), segments=(1, 3),
                      unpermute_split=(0, 1, 2))
TWO_PASS = [dict(zip(TWO_PASS_KNOBS, c)) for c in (
    (0, 0, 3, 3, 2), (0, 0, 12, 3, 0), (0, 1, 12, 1, 1), (1, 0, 12, 3, 2), (1, 1, 3, 1, 1),
    (1, 1, 3, 3, 0), (1, 0, 3, 1, 0), (0, 1, 3, 1, 2))]


def test_two_pass_selection_is_pairwise():
    for anchor in ("scatter_split", "group_bits"):
        for other in TWO_PASS_KNOBS:
            if other == anchor:
                continue
            seen = {(t[anchor], t[other]) for t in TWO_PASS}
            assert seen == set(itertools.product(TWO_PASS_KNOBS[anchor], TWO_PASS_KNOBS[other])), (anchor, other)


@pytest.mark.gpu
@pytest.mark.parametrize("tune", TWO_PASS, ids=lambda t: "-".join(f"{k}={v}" for k, v in t.items()))
def test_two_pass_shapes(tune):
    run_shapes(1 << 21, dict(tune, hot_threshold=64), want_tokens=False)


# ------------------------------------------------------------------ escape fix-up
@functools.lru_cache(maxsize=None)
def escape_case():
    """A token bucket under time regression (test_gpu_hot.py::test_hot_tb_time_regression) whose
    refill rate turns a step back in time into a balance far below zero."""
    lims = [[rl_amd.TB, 30, 20_000, 100_000.0]]
    tr = hot_trace(14, 140_000, 5_000, 0.5, [0], 60_000, regress=True)
    want = COracle(lims).run(*tr, want_tokens=False)
    return lims, tr, want


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [1 << 14, 1 << 22], ids=["one_pass", "two_pass"])
@pytest.mark.parametrize("unpermute_split", [0, 1])
def test_escape_fixup(unpermute_split, capacity):
    # remaining below -3 does not fit the packed result: it comes back through the side array
    lims, tr, want = escape_case()
    n = len(tr[0]) // 2                           # a full unpermute tile and a ragged one per batch
    for b in (slice(0, n), slice(n, 2 * n)):
        assert (want[1][b] < -3).any()
    e = rl_amd.Engine(max_batch=1 << 17, capacity=capacity)
    e.add_limiter(*lims[0])
    e.tune("hot_threshold", 4096)
    e.tune("unpermute_split", unpermute_split)
    got = [[], []]
    for b in (slice(0, n), slice(n, 2 * n)):
        a, r, _, st = e.execute(*(x[b] for x in tr), want_tokens=False)
        assert st == rl_amd.RL_OK, rl_amd.strerror(st)
        got[0].append(a); got[1].append(r)
    e.close()
    assert_same((np.concatenate(got[0]), np.concatenate(got[1]), None), want, f"escape split {unpermute_split}")
