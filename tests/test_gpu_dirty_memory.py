"""The engine on dirty device memory: every allocation of the library filled with a chosen byte
before use (rl_debug_alloc_fill), and every result still bit-exact.

Only a handful of buffers are cleared explicitly; everything else relies on a kernel writing each
word before another kernel reads it (DESIGN §7a argues that per buffer). A fresh process mostly
sees zero pages, so an ordinary run cannot tell "written first" from "happened to be zero"; late in
a long process the memory is recycled from earlier engines. The fills:
  0x00  the control: it must equal the unfilled run word for word;
  0xA5  every count and index implausible (0xA5A5A5A5 records, slots, tiles);
  0xFF  kNone, the empty-list sentinel and the largest count.
Under each fill, engines built while it is on run the life cases (tests/life_cases.py) and the
smallest parametrisation of the existing path drivers, called as they are, with the assertions
those drivers already make against the oracle and their models."""
import numpy as np
import pytest

import rl_amd
import test_gpu_engine_life as life
import test_gpu_hot
import test_gpu_migrate
import test_gpu_partition_shapes as shapes
import test_gpu_shrink
import test_gpu_snapshot
import test_gpu_walk

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xA5, 0xFF)
# life cases 1, 2 (both tables), 4, 5, 7, 8 and 9 (the queries ride on case 1: sizes-queries)
LIFE = ("sizes-split1", "sizes-device", "hot-one-pass", "hot-two-pass", "passes", "widths", "pipeline",
        "solo")


@pytest.fixture(params=FILLS, ids=lambda b: f"fill{b:02x}")
def fill(request):
    try:
        rl_amd.debug_alloc_fill(request.param)
        yield request.param
    finally:
        rl_amd.debug_alloc_fill(None)


def same_words(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", LIFE)
def test_life_case(fill, name):
    got = life.run_case(name)                     # (asserts every batch against the oracle)
    if fill == 0x00:
        rl_amd.debug_alloc_fill(None)             # the control equals the unfilled run word for word
        plain = life.run_case(name)
        assert len(plain) == len(got)
        for i, (p, g) in enumerate(zip(plain, got)):
            assert all(same_words(x, y) for x, y in zip(p, g)), f"{name} batch {i}"


def test_queries_between_batches(fill):
    life.run_queries_case()


def test_partition_shapes_one_pass(fill):
    shapes.run_shapes(1 << 14, dict(scatter_split=1, wide_records=0, unpermute_split=1), want_tokens=False)


def test_partition_shapes_two_pass(fill):
    shapes.run_shapes(1 << 21, dict(shapes.TWO_PASS[3], hot_threshold=64), want_tokens=False)


def test_walk_tables_come_up_mid_life(fill):
    # the 512 MiB of allow-walk tables are allocated once a batch has wanted a walk: dirty, mid-life
    test_gpu_walk.test_walk_with_peeks_and_resets("sw")


def test_hot_two_keys_one_region(fill):
    test_gpu_hot.test_hot_two_keys_one_region("tb", 17)


def test_snapshot_restore_round_trip(fill):
    test_gpu_snapshot.test_a_clone_decides_as_the_original()


def test_shrink(fill):
    test_gpu_shrink.test_shrink_keeps_the_keyspace()


def test_migrate_copy_put(fill):
    test_gpu_migrate.test_moved_keys_decide_as_one_engine(1)


def test_the_fill_reaches_fresh_allocations():
    """The hook itself, observed on memory the library does not initialise: a fresh allocation made
    the way every buffer is made (rl_debug_fetch "alloc_probe") holds the fill byte in every byte
    while a fill is on, for sizes below and above a page; an invalid byte is refused; and the bin
    totals beyond a batch's own bins, which the engine zeroes itself at creation, read zero
    whatever the fill."""
    with pytest.raises(rl_amd.RlError):
        rl_amd.debug_alloc_fill(256)
    with pytest.raises(rl_amd.RlError):
        rl_amd.debug_alloc_fill(-2)
    try:
        for b in (0xA5, 0xFF, 0x00, 0x3C):
            rl_amd.debug_alloc_fill(b)
            e = rl_amd.Engine(max_batch=1 << 12, capacity=1 << 10)
            for nbytes in (1, 16, 4097, 1 << 20):
                got = e.debug_alloc_probe(nbytes)
                assert got.shape == (nbytes,) and (got == b).all(), (b, nbytes, np.unique(got)[:4])
            e.add_limiter(rl_amd.TB, 5, 1000, 1.0)
            k = rl_amd.mix64(np.arange(100, dtype=np.uint64))
            a, r, t, st = e.execute(k, np.ones(100, np.int32), np.full(100, life.lc.T0 * life.lc.NS, np.int64))
            assert st == rl_amd.RL_OK and a.all()
            bt = e.debug_bin_totals()
            assert int(bt.sum()) == 100 and not bt[rl_amd.MIN_REGIONS:].any()
            e.close()
        rl_amd.debug_alloc_fill(0x77)
        rl_amd.debug_alloc_fill(None)               # off again: the next allocation is not filled with 0x77
        e = rl_amd.Engine(max_batch=1 << 12, capacity=1 << 10)
        assert not (e.debug_alloc_probe(1 << 20) == 0x77).all()
        e.close()
    finally:
        rl_amd.debug_alloc_fill(None)
