"""CPU check of the inputs of tests/test_gpu_result_widths.py: the oracle's answer to each edge
value's request set really contains every value the GPU test is about, so the generator cannot
silently stop producing one."""
import numpy as np
import pytest

from test_gpu_result_widths import A, BIG, PEEK, REGRESS, WIDTHS, reference, request_set


@pytest.mark.parametrize("m", list(WIDTHS))
def test_request_set_reaches_every_value(m):
    """On the oracle's output alone: the generator cannot silently stop producing a value."""
    (keys, permits, now, lim, op), n_main = request_set(m)
    wa, wr, wt = reference(m)
    assert 4000 <= len(keys) <= 1 << 16
    for algo in (0, 1):
        s = lim == algo
        assert (wr[s] == m).any() and (wr[s] == m - 1).any(), algo
    tb = lim == 1
    assert (wr[tb] == 1).any() and ((wr[tb] == 0) & (wa[tb] == 1)).any()
    if m <= 125:                                    # a sliding window counts requests: reachable
        sw = lim == 0                               # only for a small max
        assert (wr[sw] == 1).any() and ((wr[sw] == 0) & (wa[sw] == 1)).any()
        assert ((wr[sw] == 0) & (wa[sw] == 0) & (op[sw] == A)).any()
    assert ((wr == -1) & tb & (permits == m + 1)).any()            # the status: permits > max
    assert ((wr == -2) & ~(tb & (permits == 1) & (op <= PEEK))).sum() == 30    # the status: invalid
    for d in REGRESS:                                              # the balances
        assert ((wr == -d) & tb & (permits == 1) & (wa == 0)).sum() >= 8, d
        assert (wt[tb & (wr == -d)] == -float(d)).any(), d
    assert (wr[n_main:] < -(1 << 31)).sum() == 8 and (wr[:n_main] >= -1000).all()
    for p in BIG:
        s = (permits == p) & (op == A)
        assert s.sum() >= 2 and (wa[s].all() if p <= m else not wa[s].any()), p
    for h in (0, 1):                                               # a hot key per limiter
        k, c = np.unique(keys[lim == h], return_counts=True)
        assert c.max() >= 700
