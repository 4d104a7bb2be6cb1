"""CPU checks of the inputs of tests/test_gpu_window_classes.py (tests/window_cases.py): every
window is of the class it is listed under, and every fma-class and divide-class trace really
depends on the last bit of the window fraction: replayed with the bare multiply r * (1 / w) in
place of the true quotient, at least MIN_DIFF requests get another (allowed, remaining). That is
a condition on the inputs, not a tolerance: a kernel that took the one-multiply branch for such a
window would answer those requests wrongly. Multiply-class windows have no such remainder (the
product is the quotient for every r), so only their class is asserted."""
import importlib.util
import os

import numpy as np
import pytest

import window_cases as wc
from oracle.coracle import COracle

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("retry_after_model",
                                               os.path.join(_ROOT, "tools", "retry_after_model.py"))
rm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rm)

MIN_DIFF = 16
CLASS_FLAGS = {"mul": rm.LF_MUL, "fma": rm.LF_FMA, "div": 0}


@pytest.mark.parametrize("w", wc.WINDOWS)
def test_window_is_of_its_class(w):
    if w <= 65_536:
        assert rm.pct_flags(w) == CLASS_FLAGS[wc.window_class(w)], w
    else:
        assert w > 1 << 22 and wc.window_class(w) == "div"        # the engine divides above 2^22 ms
        assert w <= 1_073_741_823                                 # RL_MAX_WINDOW_MS


@pytest.mark.parametrize("w", wc.MUL_WINDOWS)
def test_multiply_class_has_no_discriminating_remainder(w):
    r = np.arange(w, dtype=np.float64)
    assert np.array_equal(r * (1.0 / w), r / w)
    for _, P, _ in wc.FILLS:
        assert wc.mul_wrong(w, P).size == 0


@pytest.mark.parametrize("epoch", [False, True], ids=["t0", "epoch"])
@pytest.mark.parametrize("w", wc.FMA_WINDOWS + wc.DIV_WINDOWS)
def test_trace_depends_on_the_fraction(w, epoch):
    tr = wc.window_trace(w, epoch)
    lims = wc.limiters(w)
    a_true, r_true = wc.replay(lims, tr, multiply=False)
    a_mul, r_mul = wc.replay(lims, tr, multiply=True)
    diff = int(((a_true != a_mul) | (r_true != r_mul)).sum())
    n_allowed = int((a_true != a_mul).sum())
    assert diff >= MIN_DIFF, f"w={w} epoch={epoch}: {diff} of {len(tr[0])} requests differ " \
                             f"({n_allowed} in allowed)"
    # from T0 the "limit" keys reach max in the fill window, so decisions differ too (near the
    # epoch the fill window reads its own bucket twice and stops short of max)
    assert epoch or n_allowed >= 1, f"w={w}: {diff} requests differ, none in allowed"
    # the replay with the true quotient is the oracle's answer
    want = COracle(lims).run(*tr)
    assert np.array_equal(a_true, want[0]) and np.array_equal(r_true, want[1]), (w, epoch)


@pytest.mark.parametrize("epoch", [False, True], ids=["t0", "epoch"])
@pytest.mark.parametrize("w", wc.WINDOWS)
def test_trace_shape(w, epoch):
    tr = wc.window_trace(w, epoch)
    n = len(tr[0])
    assert 4096 <= n <= wc.MAX_REQUESTS
    ms = tr[2] // wc.NS
    assert np.all(np.diff(ms) >= 0)
    t0 = wc.start_ms(w, epoch)
    assert ms[0] >= t0 and (not epoch or ms[0] < w)
    win = (ms - t0) // w
    assert {0, 1, 2} <= set(np.unique(win).tolist())               # fill, probe, probe
    # a same-key run of 64 consecutive requests (of its key) that crosses a window boundary
    k = wc.fill_key(101)
    mine = ms[tr[0] == k][:64 * 5]
    assert any(len(np.unique(mine[i:i + 64] // w)) > 1 for i in range(0, len(mine) - 63, 64))
    cuts = wc.batch_cuts(tr, 3)
    assert len(cuts) >= 4 and cuts[0] == 0 and cuts[-1] == n and np.all(np.diff(cuts) > 0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert ms[b - 1] - ms[a] < wc.SPAN_MS


@pytest.mark.parametrize("w", list(wc.WALK_CASES))
def test_walk_trace_depends_on_the_fraction(w):
    """The allow-walk traces (window_cases.walk_trace). For the windows of WALK_DISCRIMINATES the
    batch that walks (the last) holds requests whose decision the bare multiply would change: one
    is enough for a walk that multiplied to be told apart, four are asked for. For the others
    (the multiply class, and 24 ms, see WALK_DISCRIMINATES) no answer changes: those cases check
    the walk's parity with the chunk path only. The count is printed."""
    lims, tr, cuts = wc.walk_trace(w)
    assert len(cuts) == 4 and len(tr[0]) <= wc.MAX_REQUESTS
    ms = tr[2] // wc.NS
    for a, b in zip(cuts[1:-1], cuts[2:]):
        assert ms[b - 1] - ms[a] < 1 << 17                         # kWalkSpan
    a_true, r_true = wc.replay(lims, tr, multiply=False)
    a_mul, r_mul = wc.replay(lims, tr, multiply=True)
    last = slice(cuts[2], cuts[3])
    diff = int((a_true[last] != a_mul[last]).sum())
    if w in wc.WALK_DISCRIMINATES:
        assert diff >= 4, f"w={w}: {diff} decisions of the walking batch differ"
    else:
        assert wc.window_class(w) == "mul" or w == 24
        assert diff == 0 and np.array_equal(r_true, r_mul), f"w={w}: {diff} decisions differ"
    want = COracle(lims).run(*tr)
    assert np.array_equal(a_true, want[0]) and np.array_equal(r_true, want[1])
