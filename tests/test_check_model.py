"""The Python restatement of the table check's rules (check_cases.check_model) against tables whose
answer is known by construction: healthy tables built by the placement model report nothing, and
every corruption reports exactly its class, with the predicted count and first position. The
GPU tests (test_gpu_check.py) then hold the kernel to this model. No device, no library."""
import numpy as np
import pytest

import check_cases as cc

CASES = cc.structural_cases()
KNOWN = [c for c in CASES if c[3] is not None]


@pytest.mark.parametrize("algo,cache", [(cc.SW, False), (cc.SW, True), (cc.TB, False)])
def test_healthy_tables_report_nothing(algo, cache):
    for seed in (1, 2):
        t = cc.healthy_table(seed, algo, cache)
        rep = cc.check_model(t, algo)
        assert rep["bad_slots"] == 0 and not any(rep["violations"])
        assert rep["first"] == [cc.NONE] * cc.CLASSES
        assert (rep["regions"], rep["slots"]) == (8, 8 * 256)
        assert rep["used_slots"] == sum(cc.FILLS) == rep["state_slots"] + rep["tombstones"]
        assert rep["tombstones"] > 0 and (rep["cache_words"] > 0) == cache


@pytest.mark.parametrize("case", KNOWN, ids=[c[0] for c in KNOWN])
def test_each_corruption_reports_exactly_its_class(case):
    _, algo, t, found = case
    rep, want = cc.expect(t, algo, found)
    assert rep == want


def test_the_case_list_covers_every_checked_class():
    seen = set()
    for _, _, _, found in KNOWN:
        seen |= {c for c in found if c != "bad"}
    assert seen == {cc.WRONG_REGION, cc.UNREACHABLE, cc.DUPLICATE, cc.DEAD_MARK, cc.SW_START,
                    cc.SW_OFFSET, cc.TB_FLAGS}


def test_a_full_region_and_the_wrap():
    rng = np.random.default_rng(5)
    t, found = cc.full_region(rng)
    assert found == {} and cc.check_model(t, cc.SW)["used_slots"] == 256
    # the same region with one slot freed: most of its keys are now behind a free slot
    t.free(6, 100)
    assert cc.check_model(t, cc.SW)["violations"][cc.UNREACHABLE] > 100
    t, found = cc.corrupt_unreachable(cc.Table(), rng, r=1, home=252)
    assert found == {cc.UNREACHABLE: (2, 1 << 8 | 0)}            # slots 0 and 1, behind the hole at 255


def test_sliding_window_values():
    w = cc.W
    ok = lambda a, b, c, x=0: cc.slot_values(cc.SW, w, 9, a, b, c, x)  # noqa: E731
    assert ok(cc.T0, 3, w - 1) == set()
    assert ok(cc.T0 + 1, 3, 0) == {cc.SW_START}
    assert ok(cc.T0 + 1, 0, 0) == set()                              # a tombstone's stale start
    assert ok((-2 * w) & cc.M64, 1, (-(w - 1)) & 0xFFFFFFFF) == set()  # now < 0: offsets in (-w, 0]
    assert ok((-2 * w - 1) & cc.M64, 1, 0) == {cc.SW_START}
    assert ok(cc.T0, 1, w) == {cc.SW_OFFSET}
    assert ok(cc.T0, 1, (-w) & 0xFFFFFFFF) == {cc.SW_OFFSET}
    assert ok(cc.T0, 1 << 32, w << 32) == {cc.SW_OFFSET}
    assert ok(cc.T0, 1 << 32, w) == set()                            # the empty bucket's offset is free
    assert ok(cc.T0, 0xFFFFFFFF, 0) == set()                         # SW_COUNT is not checked
    assert ok(cc.T0, 1, cc.DEAD) == set()                            # offsets (2, 0)


def test_token_bucket_values():
    tb = lambda tag, a, b, c, x=0: cc.slot_values(cc.TB, cc.W, tag, a, b, c, x)  # noqa: E731
    assert tb(9, cc.f64_bits(3.5), cc.T0, 1) == set()
    assert tb(9, cc.f64_bits(float("nan")), cc.T0, 1) == set()       # TB_TOKENS is not checked
    assert tb(9, cc.f64_bits(-1.0), cc.T0, 1) == set()
    assert tb(9, 0, 0, 0) == set()
    assert tb(0, 0, 0, cc.DEAD) == set()
    assert tb(9, 0, 0, cc.DEAD) == {cc.DEAD_MARK}
    assert tb(0, 0, 0, cc.DEAD, x=1) == {cc.DEAD_MARK}
    assert tb(9, 1, 1, 3) == {cc.TB_FLAGS}
    assert tb(9, 1, 1, 1 << 40) == {cc.TB_FLAGS}


def test_ranges_add_up():
    t = cc.random_garbage(cc.healthy_table(3, cc.SW, True), np.random.default_rng(3), 80)
    whole = cc.check_model(t, cc.SW)
    assert whole["bad_slots"] > 0
    for cut in (0, 1, 3, 8):
        lo = cc.check_model(t, cc.SW, region_begin=0, region_count=cut)
        hi = cc.check_model(t, cc.SW, region_begin=cut)
        assert cc.add_reports(lo, hi) == whole
    beyond = cc.check_model(t, cc.SW, region_begin=8)
    assert beyond == cc.empty_report(0, 0)
