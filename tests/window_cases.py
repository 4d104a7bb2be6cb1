"""Sliding-window traces that tell the three implementations of the window fraction apart.

The fraction (double)(now % w) / w of getCurrentCount (SlidingWindowRateLimiter.java:170-171) is
computed by the kernels in one of three ways, chosen per limiter by the host (rl_engine.cpp
pct_flags): one multiply by 1/w, that multiply plus an fma correction, or a true division (every
window above 2^22 ms). A trace tests a class only if the last bit of the fraction changes an
answer. For a key with P allowed requests in the previous window, a request at remainder r does
that when P * (w - r) / w is an integer: there the rounding of the fraction decides the
truncation of the estimate. The traces below fill keys to a chosen P in one window and probe them
in the next two at those remainders, first of all at the ones where the bare multiply is wrong
(`mul_wrong`), with acquires (keys at their limit: `allowed` depends on it) and peeks.

Plain numpy / Python, no GPU: tests/test_window_cases_model.py checks the classes and counts, per
trace, the requests whose (allowed, remaining) differ between the true quotient and the bare
multiply (`replay`); tests/test_gpu_window_classes.py runs the traces through every kernel path.
"""
import math

import numpy as np

import rl_amd

NS = 1_000_000
T0 = 1_700_000_000_000
SW = 0
OP_ACQUIRE, OP_PEEK, OP_RESET = 0, 1, 2

MUL_WINDOWS = (16, 25, 59, 1024, 65_536)
FMA_WINDOWS = (24, 1000, 60_000)
DIV_WINDOWS = (4_200_000, 1_073_741_000)          # the second: just under RL_MAX_WINDOW_MS
WINDOWS = MUL_WINDOWS + FMA_WINDOWS + DIV_WINDOWS
MAX_REQUESTS = 1 << 16
SPAN_MS = 1 << 30                                  # a batch stays well inside the compact +-2^31 ms

# FILLS lists (limiter, nominal P, probes): keys filled to P allowed requests in the fill window.
# Limiter 0 has max 1000, limiter 1 max 100, limiter 2 max 7 (background traffic, a dense run).
#
# The probes of a key at a point r:
#   "limit" (P = max): as many acquires as the estimate has fallen by since the last point and one
#       more, then a peek. The key is at its limit at every point, so the last acquire's
#       `allowed` hangs on the fraction.
#   "acquire": two acquires and a peek. `remaining` hangs on the fraction, less and less as curr
#       grows, because the sum prev * weight + curr is rounded again.
#   "peek": two peeks. curr stays 0, so every remainder the multiply gets wrong shows.
#
# For a window w below the nominal value, P and the maxima are its largest multiple of w
# (`fill_count`). P * (w - r) / w is then an integer at every r. Only so can a window as small
# as 24 ms reach the remainders its multiply gets wrong.
MAXES = (1000, 100, 7)
FILLS = ((0, 1000, "limit"), (0, 500, "acquire"), (0, 500, "peek"), (0, 250, "peek"),
         (1, 100, "limit"), (1, 50, "acquire"), (1, 50, "peek"))
POINTS_PER_KEY = 300


def fill_count(nominal, w):
    return nominal // w * w if w <= nominal else nominal


def window_class(w):
    return "mul" if w in MUL_WINDOWS else "fma" if w in FMA_WINDOWS else "div"


def limiters(w, cache_ttl=0):
    """The three limiters of a window's traces; cache_ttl > 0: with the local cache on."""
    tail = [0, cache_ttl] if cache_ttl else []
    return [[SW, fill_count(m, w) if m > 7 else m, w, 0.0] + tail for m in MAXES]


def fill_key(i):
    return int(rl_amd.mix64(np.array([i], np.uint64) + np.uint64(0xF111 << 32))[0])


def points(w, P):
    """The remainders 0 < r < w at which P * (w - r) / w is an integer."""
    step = w // math.gcd(w, P)
    return np.arange(step, w, step, dtype=np.int64)


def estimates(w, P, r, curr=0):
    """d2l(P * (1 - r / w) + curr) with the true quotient and with the bare multiply r * (1 / w)."""
    r = np.asarray(r, np.float64)
    inv = 1.0 / float(w)
    true = np.trunc(float(P) * (1.0 - r / float(w)) + np.asarray(curr, np.float64)).astype(np.int64)
    mul = np.trunc(float(P) * (1.0 - r * inv) + np.asarray(curr, np.float64)).astype(np.int64)
    return true, mul


def mul_wrong(w, P, at_limit=False):
    """Those of points(w, P) at which the bare multiply gives another estimate than the division;
    at_limit: with the current bucket at P - P * (w - r) / w, as for a key at its limit P (the sum
    prev * weight + curr is rounded again, which hides the fraction's last bit once the weighted
    count is in a lower binade than the sum)."""
    r = points(w, P)
    true, mul = estimates(w, P, r, P - P * (w - r) // w if at_limit else 0)
    return r[true != mul]


def probe_points(w, P, rng, limit=POINTS_PER_KEY, at_limit=False):
    """At most `limit` of points(w, P): the ones the bare multiply gets wrong first, the rest drawn
    at random."""
    r = points(w, P)
    if len(r) <= limit:
        return r
    bad = mul_wrong(w, P, at_limit)[:limit]
    rest = np.setdiff1d(r, bad)
    more = rng.choice(rest, limit - len(bad), replace=False) if len(bad) < limit else rest[:0]
    return np.sort(np.concatenate([bad, more]))


def start_ms(w, epoch):
    return 0 if epoch else (T0 // w + 1) * w


def cycles(w):
    return 1 if w >= 60_000 else 4


def window_trace(w, epoch=False, seed=0):
    """(keys, permits, now_ns, limiter, op) in arrival order. Per cycle of three windows, from
    `start_ms`: window 0 fills the FILLS keys to P, windows 1 and 2 probe them at probe_points;
    two dense same-key runs cross the boundary of windows 1 | 2
    (several requests per ms, so a 64-request group holds the roll-over); background keys with
    peeks and resets lie over all of it. epoch: the first timestamp is 0, so the first window has
    0 <= now < w (prev_start == curr_start under Java's truncating division)."""
    rng = np.random.default_rng(seed * 1000 + w % 997 + (500 if epoch else 0))
    t_start = start_ms(w, epoch)
    cols = [[], [], [], [], []]                     # key, permits, ms, limiter, op

    def add(key, permits, ms, lim, op):
        ms = np.asarray(ms, np.int64)
        n = len(ms)
        cols[0].append(np.full(n, key, np.uint64) if np.isscalar(key) else np.asarray(key, np.uint64))
        cols[1].append(np.broadcast_to(np.asarray(permits, np.int32), (n,)))
        cols[2].append(ms)
        cols[3].append(np.full(n, lim, np.uint16) if np.isscalar(lim) else np.asarray(lim, np.uint16))
        cols[4].append(np.broadcast_to(np.asarray(op, np.uint8), (n,)))

    for c in range(cycles(w)):
        w0 = t_start + 3 * w * c
        for i, (lim, P, mode) in enumerate(FILLS):
            key, P = fill_key(i), fill_count(P, w)
            add(key, 1, w0 + np.sort(rng.integers(0, w, P)), lim, OP_ACQUIRE)
            r = probe_points(w, P, rng, at_limit=mode == "limit")
            if mode == "limit":
                freed = np.diff(np.concatenate([[0], r])) * P // w
                reps = np.minimum(freed + 1, 63) + 1
            else:
                reps = np.full(len(r), 3 if mode == "acquire" else 2)
            op = np.full(int(reps.sum()), OP_PEEK if mode == "peek" else OP_ACQUIRE, np.uint8)
            op[np.cumsum(reps) - 1] = OP_PEEK
            for wi in (1, 2):
                add(key, 1, np.repeat(w0 + wi * w + r, reps), lim, op)
        b = w0 + 2 * w                               # the boundary of windows 1 | 2
        add(fill_key(100), rng.integers(1, 3, 300), b - min(150, 2 * w) + np.arange(300), 1, OP_ACQUIRE)
        add(fill_key(101), 1, b - min(40, 2 * w) + 3 + np.arange(320) // 4, 2, OP_ACQUIRE)
        n_bg = 4000
        ranks = rng.integers(0, 1500, n_bg)
        op = np.zeros(n_bg, np.uint8)
        u = rng.random(n_bg)
        op[u < 0.04] = OP_PEEK
        op[u < 0.01] = OP_RESET
        add(rl_amd.mix64(ranks.astype(np.uint64) + np.uint64(0xB6 << 40)), rng.integers(1, 4, n_bg),
            w0 + rng.integers(0, 3 * w, n_bg), (ranks % 3).astype(np.uint16), op)
    keys, permits, ms, lim, op = (np.concatenate(x) for x in cols)
    o = np.argsort(ms, kind="stable")
    assert len(o) <= MAX_REQUESTS and ms.min() >= t_start
    return (keys[o], permits[o].astype(np.int32), ms[o] * NS, lim[o], op[o])


def batch_cuts(tr, batches=3, span_ms=SPAN_MS):
    """Cut indices [0, ..., n] of at least `batches` batches, none spanning span_ms or more."""
    ms = tr[2] // NS
    n = len(ms)
    per = -(-n // batches)
    cuts = [0]
    while cuts[-1] < n:
        s = cuts[-1]
        by_time = int(np.searchsorted(ms, ms[s] + span_ms, side="left"))
        cuts.append(min(s + per, by_time, n))
    return cuts


def fill_prefix(tr, w, epoch):
    """The requests of the first fill window alone, and the start of the window after it."""
    w1 = start_ms(w, epoch) + w
    n = int(np.searchsorted(tr[2], w1 * NS, side="left"))
    return tuple(x[:n] for x in tr), w1


# ---------------------------------------------------------------- the model
def replay(lims, tr, multiply):
    """Sequential replay of a sliding-window trace (no local cache) as the oracle decides it
    (oracle/rl_oracle.py _current_count / _sw_acquire), with the window fraction as the true
    quotient or, `multiply`, as the bare product r * (1 / w). Returns (allowed, remaining)."""
    keys, permits, now_ns, lim, op = tr
    n = len(keys)
    allowed, remaining = np.zeros(n, np.uint8), np.zeros(n, np.int64)
    state = {}                                       # (limiter, key) -> {window start: [count, expire]}
    kl, pl, tl, ll, ol = keys.tolist(), permits.tolist(), (now_ns // NS).tolist(), lim.tolist(), op.tolist()
    for i in range(n):
        _, mx, w, _ = lims[ll[i]][:4]
        now = tl[i]
        s = state.setdefault((ll[i], kl[i]), {})
        curr_start = now // w * w                   # now >= 0: truncation = floor
        d = now - w
        prev_start = (d // w if d >= 0 else -((-d) // w)) * w
        r = float(now - curr_start)
        pw = 1.0 - (r * (1.0 / float(w)) if multiply else r / float(w))

        def get(start):
            b = s.get(start)
            return b[0] if b is not None and not now > b[1] else 0

        if ol[i] == OP_RESET:
            s.pop(curr_start, None)
            s.pop(prev_start, None)
            continue
        est = int(float(get(prev_start)) * pw + float(get(curr_start)))
        if ol[i] == OP_ACQUIRE and est + pl[i] <= mx:
            nc = get(curr_start) + 1
            s[curr_start] = [nc, now + w]
            allowed[i] = nc <= mx
            est = int(float(get(prev_start)) * pw + float(nc))
        remaining[i] = max(0, mx - est)
    return allowed, remaining


# ---------------------------------------------------------------- allow walks
# window: (span of the two dense batches in ms, max). Each batch spans less than kWalkSpan
# (2^17 ms), so the walk tables are built.
WALK_CASES = {16: (1000, 9), 25: (1000, 14), 59: (1000, 31), 1024: (4000, 101),
              65_536: (120_000, 150), 24: (800, 24), 1000: (4000, 100), 60_000: (120_000, 200),
              4_200_000: (120_000, 250)}
# The cases whose walking batch a bare multiply would decide differently. The multiply-class
# windows cannot be told apart by definition. Nor can 24 ms: a key at its limit keeps the sum
# prev * weight + curr at max = 24, whose rounding hides the fraction's last bit. That case checks
# the walk's parity only; 1000 and 60 000 stand for the fma class.
WALK_DISCRIMINATES = (1000, 60_000, 4_200_000)


def walk_trace(w, seed=0):
    """One dense key at its limit, for the hot chains' allow walk: (limiters, trace, cuts).

    Batch 1 fills the key to max in one window. Batches 2 and 3 split the span after it and hold
    the fewest requests of the key that the walk's density rule admits, a few per ms. The engine
    allocates the walk tables once a batch has wanted a walk, so the third batch is the one that
    walks. Among the key's requests are three at every instant at which the bare multiply gets
    the estimate of a key at its limit wrong.

    max is chosen so that the density rule holds at this size (rl_hot.hpp walk_dense: per batch,
    expected allows max * (span / w + 2) <= 2.5 per 64 records). For a window longer than the
    span, the walking batch lies where the wrong instants are densest.

    The largest window has no walk case. Below 64K requests the rule admits max <= 1250, and then
    its estimate falls by one every 859 s or more, beyond any walk table."""
    rng = np.random.default_rng(7000 + seed + w % 997)
    span, mx = WALK_CASES[w]
    lims = [[SW, mx, w, 0.0], [SW, 5, w, 0.0]]
    w0 = start_ms(w, False)
    hot = fill_key(200)
    bad = mul_wrong(w, mx, at_limit=True)
    off = 0
    if w > span and len(bad):
        per = np.searchsorted(bad, bad + span // 2) - np.arange(len(bad))   # per half span:
        off = max(int(bad[int(np.argmax(per))]) - 500 - span // 2, 0)      # the walking batch's
    b2 = w0 + w + off
    t = np.arange(span, dtype=np.int64)
    at = t[np.isin((off + t) % w, bad)][:1000]
    # per dense batch: 0.4 chunks of 64 records per expected allow (walk_dense), and a fifth more
    n_hot = 2 * int(0.4 * mx * (span / 2 / w + 2) * 64 * 1.2)
    n_bg = 3_000
    parts = []
    parts.append((np.full(mx, hot, np.uint64), np.ones(mx, np.int32),
                  w0 + np.sort(rng.integers(0, w, mx)), np.zeros(mx, np.uint16)))
    bg = rl_amd.mix64(rng.integers(0, 800, 1000).astype(np.uint64) + np.uint64(0xB7 << 40))
    parts.append((bg, rng.integers(1, 3, 1000).astype(np.int32), w0 + np.sort(rng.integers(0, w, 1000)),
                  np.ones(1000, np.uint16)))
    n1 = mx + 1000
    t_hot = np.concatenate([rng.integers(0, span, n_hot), np.repeat(at, 3)])
    parts.append((np.full(len(t_hot), hot, np.uint64), rng.integers(1, 3, len(t_hot)).astype(np.int32),
                  b2 + t_hot, np.zeros(len(t_hot), np.uint16)))
    bg = rl_amd.mix64(rng.integers(0, 800, n_bg).astype(np.uint64) + np.uint64(0xB7 << 40))
    parts.append((bg, rng.integers(1, 3, n_bg).astype(np.int32), b2 + rng.integers(0, span, n_bg),
                  (rng.integers(0, 2, n_bg)).astype(np.uint16)))
    keys, permits, ms, lim = (np.concatenate([p[i] for p in parts]) for i in range(4))
    o = np.concatenate([np.argsort(ms[:n1], kind="stable"), n1 + np.argsort(ms[n1:], kind="stable")])
    n = len(o)
    assert n <= MAX_REQUESTS
    tr = (keys[o], permits[o], ms[o].astype(np.int64) * NS, lim[o], np.zeros(n, np.uint8))
    half = n1 + int(np.searchsorted(ms[o][n1:], b2 + span // 2))
    return lims, tr, [0, n1, half, n]
