"""Ordered batches on the CPU oracles: for every K-run decision trace of tests/order_cases.py,
deciding in array order and deciding in time order differ for every limiter (so a check of an
ordered batch against these traces cannot pass by ignoring the order), and the C oracle equals the
Python oracle on the time-sorted stream."""
import numpy as np
import pytest

import order_cases as oc
from oracle.coracle import COracle
from oracle.rl_oracle import PyOracle


def py_run(limiters, batches):
    o = PyOracle()
    for algo, mx, w, rate, ttl in limiters:
        o.add_limiter(algo, mx, w, rate, local_cache_ttl_ms=ttl)
    res = []
    for keys, permits, ns, lim, ops in batches:
        a, r, t = o.run(keys, permits, ns, lim, ops)
        res.append((np.array(a, np.uint8), np.array(r, np.int64), np.array(t, np.float64)))
    return res


def c_run(limiters, batches):
    o = COracle()
    for algo, mx, w, rate, ttl in limiters:
        o.add_limiter(algo, mx, w, rate, local_cache_ttl_ms=ttl)
    res = [o.run(*b)[:3] for b in batches]
    o.close()
    return res


def check_trace(limiters, batches):
    plain = py_run(limiters, batches)
    perms, sorted_batches = zip(*[oc.sort_batch(b) for b in batches])
    in_time = py_run(limiters, sorted_batches)
    c_time = c_run(limiters, sorted_batches)
    differ = np.zeros(len(limiters), np.int64)
    for b, (perm, (pa, _, _), (ta, tr, tt), (ca, cr, ct)) in enumerate(zip(perms, plain, in_time, c_time)):
        assert oc.order_model(batches[b][2])[1]["descents"] > 0
        assert np.array_equal(ca, ta) and np.array_equal(cr, tr), b
        m = ~np.isnan(tt)
        assert np.array_equal(np.isnan(ct), np.isnan(tt))
        assert np.array_equal(ct[m].view(np.uint64), tt[m].view(np.uint64)), b
        (back,) = oc.scatter_back(perm, ta)
        lim = batches[b][3]
        for l in range(len(limiters)):
            differ[l] += int((back[lim == l] != pa[lim == l]).sum())
    assert np.all(differ >= 1), differ


# (the fixture builds the C oracle's library before COracle loads it)
@pytest.mark.usefixtures("coracle_lib")
@pytest.mark.parametrize("name", list(oc.TRACES))
def test_array_order_and_time_order_decide_differently(name):
    check_trace(oc.MIXES[oc.TRACES[name][0]], oc.trace_batches(name))


@pytest.mark.usefixtures("coracle_lib")
def test_hot_trace_decides_differently():
    check_trace(oc.HOT_LIMITERS, oc.hot_batches())


def test_the_model_is_a_stable_sort_by_floored_millisecond():
    ns = np.array([1_999_999, 1_000_000, -1, 0, -1_000_000, -1_000_001, 999_999], np.int64)
    assert oc.ms_of(ns).tolist() == [1, 1, -1, 0, -1, -2, 0]
    perm, hdr = oc.order_model(ns)
    assert perm.tolist() == [5, 2, 4, 3, 6, 0, 1]
    assert hdr == {"descents": 3, "min_ms": -2, "max_ms": 1, "passes": 1}
    for name in oc.PATTERNS:
        ns = oc.pattern_ns(name, 300)
        perm, hdr = oc.order_model(ns)
        ms = oc.ms_of(ns)
        assert sorted(perm.tolist()) == list(range(300))
        key = ms[perm] * 1000 + perm                        # (ms, index) strictly increasing
        assert np.all(np.diff(key) > 0), name
        if name.startswith("span"):
            want = (1 << 32) + 5 if name == "span2p32" else int(name[4:])
            assert hdr["max_ms"] - hdr["min_ms"] == want, name
    assert oc.order_model(oc.pattern_ns("sorted", 300))[1]["descents"] == 0
    # a same-millisecond pair whose nanoseconds are reversed keeps array order
    ns = oc.pattern_ns("same_ms_pairs", 300)
    assert np.all(ns[0::2] > ns[1::2]) and np.array_equal(oc.ms_of(ns)[0::2], oc.ms_of(ns)[1::2])
    pos = np.empty(300, np.int64)
    pos[oc.order_model(ns)[0]] = np.arange(300)
    assert np.all(pos[0::2] + 1 == pos[1::2])
