"""Ordered batches (a batch decided in timestamp order) restated in numpy from
their definition, with the inputs their checks share: timestamp patterns for the sort, K-run
decision traces and limiter mixes for the decisions."""
import numpy as np

SW, TB = 0, 1
DIGIT_BITS = 8                   # kOrderDigitBits (csrc/rl_order.hpp)
T0_MS = 1_700_000_000_000


def ms_of(now_ns):
    """floorDiv(now_ns, 1e6): numpy's // on int64 floors."""
    return np.asarray(now_ns, np.int64) // 1_000_000


def order_model(now_ns):
    """The time order of a batch: (perm uint32, {descents, min_ms, max_ms, passes}), descents =
    #{i >= 1 : ms[i] < ms[i-1]}; passes is the plan's count, or 0 for a batch already in time
    order."""
    ms = ms_of(now_ns)
    n = ms.shape[0]
    if n == 0:
        return np.zeros(0, np.uint32), {"descents": 0, "min_ms": 0, "max_ms": 0, "passes": 0}
    perm = np.argsort(ms, kind="stable").astype(np.uint32)
    desc = int((ms[1:] < ms[:-1]).sum())
    mn, mx = int(ms.min()), int(ms.max())
    return perm, {"descents": desc, "min_ms": mn, "max_ms": mx,
                  "passes": plan_passes(mx - mn) if desc else 0}


def plan_passes(span):
    return -(-int(span).bit_length() // DIGIT_BITS)


def plan_model(span):
    """order_plan by brute force: (passes, wide, [(shift, bits)])."""
    length = int(span).bit_length()
    passes = -(-length // DIGIT_BITS)
    digits, at = [], 0
    for i in range(passes):
        left = passes - i
        b = -(-(length - at) // left)
        digits.append((at, b))
        at += b
    return passes, length > 32, digits


def scatter_back(perm, *sorted_results):
    out = []
    for r in sorted_results:
        if r is None:
            out.append(None)
            continue
        o = np.empty_like(r)
        o[perm] = r
        out.append(o)
    return out


# ---- timestamp patterns (the sort)
def runs_ms(rng, n, k, span_ms):
    """k sorted runs of n // k (+ rest) timestamps over one interval [0, span_ms]."""
    sizes = [n // k + (1 if i < n % k else 0) for i in range(k)]
    return np.concatenate([np.sort(rng.integers(0, span_ms + 1, s)) for s in sizes]) if n else np.zeros(0, np.int64)


def with_span(rng, n, span_ms):
    """Random ms over exactly [0, span_ms] (both ends present when n >= 2)."""
    ms = rng.integers(0, span_ms + 1, n).astype(np.int64)
    if n >= 2:
        i, j = rng.choice(n, 2, replace=False)
        ms[i], ms[j] = 0, span_ms
    return ms


PATTERNS = ("sorted", "reversed", "equal", "runs2", "runs4", "runs8", "runs64", "random",
            "span0", "span255", "span256", "span257", "span65535", "span65536", "span65537", "span2p32",
            "straddle0", "same_ms_pairs")


def pattern_ns(name, n, seed=0):
    """now_ns (int64) of n requests in the named pattern."""
    rng = np.random.default_rng(seed * 1000 + len(name) * 31 + n % 977)
    sub = rng.integers(0, 1_000_000, n).astype(np.int64)
    if name == "sorted":
        ms = np.sort(rng.integers(0, 3500, n)) + T0_MS
    elif name == "reversed":
        ms = np.sort(rng.integers(0, 3500, n))[::-1].copy() + T0_MS
    elif name in ("equal", "span0"):
        ms = np.full(n, T0_MS + 17, np.int64)
    elif name.startswith("runs"):
        ms = runs_ms(rng, n, int(name[4:]), 3500) + T0_MS
    elif name == "random":
        ms = rng.integers(0, 100_000, n) + T0_MS
    elif name == "span2p32":
        ms = with_span(rng, n, (1 << 32) + 5) + T0_MS
    elif name.startswith("span"):
        ms = with_span(rng, n, int(name[4:])) + T0_MS
    elif name == "straddle0":
        # ms in [-40, 40): negative ns floor towards -inf (-1 ns is ms -1)
        ns = rng.integers(-40_000_000, 40_000_000, n).astype(np.int64)
        if n >= 2:
            ns[0], ns[1] = -1, 0
        return ns
    elif name == "same_ms_pairs":
        # neighbours share a millisecond with their ns reversed: they must keep array order
        ms = np.repeat(rng.integers(0, 50, (n + 1) // 2), 2)[:n] + T0_MS
        sub = np.where(np.arange(n) % 2 == 0, 900_000, 100).astype(np.int64)
    else:
        raise KeyError(name)
    return np.asarray(ms, np.int64) * 1_000_000 + sub


# ---- decision traces (the ordered execute): K time-sorted runs over the same interval
MIXES = {
    "sw":      [(SW, 5, 1000, 0.0, 0)],
    "tb":      [(TB, 6, 1000, 2.0, 0)],
    "swcache": [(SW, 5, 1000, 0.0, 300)],
    "mixed10": [(SW, 5, 1000, 0.0, 0), (TB, 6, 1000, 2.0, 0), (SW, 3, 700, 0.0, 0), (TB, 4, 500, 5.0, 0),
                (SW, 9, 1500, 0.0, 200), (TB, 2, 2000, 0.5, 0), (SW, 1, 400, 0.0, 0), (TB, 12, 800, 7.0, 0),
                (SW, 7, 900, 0.0, 0), (TB, 3, 1200, 1.5, 0)],
}
# (mix, K runs, requests per batch, keys, ops mix, invalid requests)
TRACES = {
    "sw_k2":       ("sw", 2, 1200, 12, False, False),
    "tb_k4":       ("tb", 4, 2080, 12, False, False),
    "swcache_k8":  ("swcache", 8, 2056, 12, False, False),
    "mixed10_k4":  ("mixed10", 4, 3001, 40, False, False),
    "ops_k8":      ("mixed10", 8, 4100, 40, True, False),
    "invalid_k4":  ("mixed10", 4, 2500, 40, True, True),
}
BATCHES = 3
BATCH_SPAN_MS = 3500             # > 2 rollovers of every window above


def trace_batches(name):
    """BATCHES consecutive batches of the named trace: each a tuple (keys u64, permits i32, now_ns
    i64, limiter u16, ops u8) whose K runs are each sorted by time over the batch's own interval;
    the batches' intervals follow each other, so state carries and no request lags a batch."""
    mix, k, n, n_keys, with_ops, with_invalid = TRACES[name]
    n_lim = len(MIXES[mix])
    rng = np.random.default_rng(sum(map(ord, name)))
    out = []
    for b in range(BATCHES):
        ms = runs_ms(rng, n, k, BATCH_SPAN_MS - 1) + T0_MS + b * BATCH_SPAN_MS
        ns = ms * 1_000_000 + rng.integers(0, 1_000_000, n)
        keys = rng.integers(1, n_keys + 1, n).astype(np.uint64)
        permits = rng.integers(1, 4, n).astype(np.int32)
        lim = (keys % n_lim).astype(np.uint16)
        ops = np.zeros(n, np.uint8)
        if with_ops:                                       # 90 / 7 / 3 %
            u = rng.random(n)
            ops[u >= 0.90] = 1
            ops[u >= 0.97] = 2
        if with_invalid:
            u = rng.random(n)
            permits[u < 0.02] = 0
            permits[(u >= 0.02) & (u < 0.03)] = -5
            lim[(u >= 0.03) & (u < 0.05)] = n_lim + 3
            ops[(u >= 0.05) & (u < 0.06)] = 7
        out.append((keys, permits, ns.astype(np.int64), lim, ops))
    return out


def hot_batches():
    """One dominant key (70 % of the requests) spread over 8 runs, on a sliding window and a token
    bucket; three batches."""
    rng = np.random.default_rng(4242)
    out = []
    n, k = 9000, 8
    for b in range(BATCHES):
        ms = runs_ms(rng, n, k, BATCH_SPAN_MS - 1) + T0_MS + b * BATCH_SPAN_MS
        ns = ms * 1_000_000 + rng.integers(0, 1_000_000, n)
        keys = np.where(rng.random(n) < 0.7, 77, rng.integers(1, 30, n)).astype(np.uint64)
        permits = rng.integers(1, 3, n).astype(np.int32)
        lim = (rng.random(n) < 0.5).astype(np.uint16)
        out.append((keys, permits, ns.astype(np.int64), lim, np.zeros(n, np.uint8)))
    return out


HOT_LIMITERS = [(SW, 400, 1000, 0.0, 0), (TB, 300, 1000, 150.0, 0)]


def sort_batch(batch):
    perm, _ = order_model(batch[2])
    return perm, tuple(x[perm] for x in batch)
