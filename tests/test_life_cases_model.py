"""The life cases (tests/life_cases.py) are meaningful, from the oracle alone (CPU, no GPU): every
batch of every case both allows and denies (a single request is exempt), a hot batch has a region
holding at least the threshold's number of records, and a "none" batch has no such region. These
are conditions on the seeds, checked here before tests/test_gpu_engine_life.py runs the cases."""
import numpy as np
import pytest

import life_cases as lc
import rl_amd


def walk(case):
    """(batch, region bits per limiter or None) along the case's steps: the region count follows
    the grow steps exactly; after a shrink (its plan depends on the table's fill) it is unknown."""
    per = case.capacity // len(case.limiters)
    bits = [lc.region_bits(per) for _ in case.limiters]
    for s in case.steps:
        if s[0] == "grow":
            bits[s[1]] = lc.grown_bits(bits[s[1]], s[2])
        elif s[0] == "shrink":
            bits[s[1]] = None
        elif s[0] == "add_limiter":
            bits.append(lc.region_bits(per))
        elif s[0] == "regions" and None not in bits:
            total = sum(1 << b for b in bits)
            assert (total > lc.MAX_ONE_PASS_REGIONS) == (s[1] == "two"), (case.name, total, s)
        elif s[0] == "batch":
            yield s[1], list(bits)


@pytest.mark.parametrize("name", list(lc.CASES))
def test_every_batch_meets_its_conditions(name):
    case, want = lc.get(name)
    assert len(want) == len(case.batches()) >= 3
    for i, ((b, bits), w) in enumerate(zip(walk(case), want)):
        n = len(b.tr[0])
        allowed = int(w[0].sum())
        if n > 1:
            assert 0 < allowed < n, f"{name} batch {i} ({b.note}): the oracle allows {allowed} of {n}"
        if b.hot_keys is not None:
            if None in bits:                      # a lower bound: a key's records share one region
                top = max(int((b.tr[0] == k).sum()) for k in b.hot_keys)
            else:
                top = max(int(c.max()) for c in lc.region_counts(b.tr, bits))
            assert top >= case.hot_thr, f"{name} batch {i}: largest region {top}"
        if b.none:
            assert None not in bits
            top = max(int(c.max()) for c in lc.region_counts(b.tr, bits))
            assert top < case.hot_thr, f"{name} batch {i}: a region holds {top} records"
        if b.cache_hits:
            before = want[i - 1][4] if i else 0
            assert w[4] > before, f"{name} batch {i}: no local-cache hit"
        assert np.all(np.diff(b.tr[2][b.tr[2] < (lc.T0 + (1 << 32)) * lc.NS]) >= 0)   # arrival order


def test_sizes_case_has_the_issues_sizes_and_alternates_balances():
    for name in ("sizes-split0", "sizes-split1", "sizes-device"):
        case, _ = lc.get(name)
        b = case.batches()
        assert [len(x.tr[0]) for x in b] == [66_049, 1, 4_097, 63, 12_801, 64, 65, 66_049]
        assert [x.want_tokens for x in b] == [True, False] * 4
        assert case.tile_items == 8 and case.capacity == 1 << 14
    assert {lc.get(n)[0].tune["scatter_split"] for n in ("sizes-split0", "sizes-split1")} == {0, 1}
    assert all(x.entry == "device" for x in lc.get("sizes-device")[0].batches())
    # some request of every invalid kind, so the status path runs too
    _, want = lc.get("sizes-split0")
    assert want[0][3] > 0


def test_hot_cases_step_every_knob_and_shift_the_hot_set():
    for name in ("hot-one-pass", "hot-two-pass"):
        case, _ = lc.get(name)
        tunes = [(s[1], s[2]) for s in case.steps if s[0] == "tune"]
        for seq in ([("hot_threshold", 0), ("hot_threshold", 256)], [("walk", 0), ("walk", 1)],
                    [("chain_split", 0)], [("route", 0), ("route", 1)], [("segments", 4), ("segments", 1)],
                    [("region_order", 0)]):
            at = [tunes.index(t) for t in seq]
            assert at == sorted(at), seq
        b = case.batches()
        # X, Y, none, X: a region hot in batch k is an ordinary, non-empty one in batch k + 1, per
        # (limiter, region): the very region the hot path marked, not merely the same key
        bits = [lc.region_bits(case.capacity // 2)] * 2
        shifts = 0
        for k in range(len(b) - 1):
            if b[k].hot_keys is not None and b[k + 1].hot_keys is not b[k].hot_keys:
                shifts += 1
                now, nxt = lc.region_counts(b[k].tr, bits), lc.region_counts(b[k + 1].tr, bits)
                for key in b[k].hot_keys:
                    l = lc.limiter_of(key)
                    r = int(rl_amd.mix64(np.array([key], np.uint64))[0] >> np.uint64(64 - bits[l]))
                    assert now[l][r] >= case.hot_thr, (name, k, l, r)
                    assert 0 < nxt[l][r] < case.hot_thr, (name, k, l, r, int(nxt[l][r]))
                    assert 0 < (b[k + 1].tr[0] == key).sum() < case.hot_thr
                    # the key comes under one limiter throughout
                    for x in (b[k], b[k + 1]):
                        assert set(x.tr[3][x.tr[0] == key].tolist()) == {l}
        assert shifts >= 6                          # X -> Y and Y -> none, three times each
        assert sum(x.hot is True for x in b) >= 6 and sum(x.hot is False for x in b) >= 2
    two = lc.get("hot-two-pass")[0].batches()
    assert sum(x.routed is True for x in two) == 7 and sum(x.routed is False for x in two) == 5
    assert all(x.hot is not None for x in two)
    assert two[0].routed is False               # nothing is listed before the first batch


def test_epoch_case_wraps_in_the_third_batch():
    for name in ("epoch", "epoch-pipelined"):
        case, _ = lc.get(name)
        kinds = [s[0] if s[0] != "tune" else s[1:] for s in case.steps]
        assert kinds == ["batch", ("hot_epoch", 0xFFFFFFFE), "batch", "batch", "batch"]
        b = case.batches()
        sets = [frozenset(int(k) for k in x.hot_keys) for x in b]
        assert sets[0] == sets[3] != sets[1] == sets[2]
        # batch 3: X's regions carry plenty of traffic below the threshold
        for key in lc.X:
            assert 100 <= (b[2].tr[0] == key).sum() < case.hot_thr
    assert lc.get("epoch-pipelined")[0].pipeline


def test_regrow_case_exceeds_the_first_batchs_headroom():
    for name in ("regrow", "regrow-wide"):
        case, _ = lc.get(name)
        n = [len(x.tr[0]) for x in case.batches()]
        assert n == [(1 << 20) + 5_000, 1_300_000, 5_000]
        assert n[1] > n[0] + n[0] // 8 and n[1] <= case.max_batch == 1 << 21
        assert case.tile_items == 0
    tunes = [s[1:] for s in lc.get("regrow-wide")[0].steps if s[0] == "tune"]
    assert tunes == [("wide_records", 1), ("wide_records", 0)]


def test_widths_case_has_a_wide_batch_smaller_than_the_one_before_and_a_far_one_between():
    case, _ = lc.get("widths")
    b = case.batches()
    assert len(b[1].tr[0]) < len(b[0].tr[0])
    span = [int(x.tr[2].max() - x.tr[2].min()) // lc.NS for x in b]
    assert span[3] > 1 << 32 and max(span[:3] + span[4:]) < 2 * lc.SPAN_MS
    assert [s[1] for s in case.steps if s[0] == "width"] == [1, 1, 4, 8]


def test_pipeline_case_flips_each_sets_sizes():
    case, _ = lc.get("pipeline")
    n = [len(x.tr[0]) for x in case.batches()]
    assert len(n) == 7 and case.pipeline
    # big, small, big, small, small, big, small over two alternating scratch sets: set 0 meets a
    # smaller batch after a larger one twice over, set 1 a larger one after two smaller ones
    big, small = max(n), min(n)
    assert [x > 4 * small for x in n] == [True, False, True, False, False, True, False]
    assert any(a > b for a, b in zip(n[0::2], n[2::2])) and any(a < b for a, b in zip(n[1::2], n[3::2]))
    assert big > 4 * lc.TILE and rl_amd.REGION_SLOTS == 256
