"""The batch report's definition (include/rl_engine.h, "batch report") restated in numpy, and the
synthetic batches the GPU tests run it on. Not used by the engine."""
import numpy as np

import rl_amd

INVALID, ERROR, ALLOWED, DENIED, PEEK, RESET = range(6)
COLS = ("invalid", "errors", "allowed", "denied", "peeks", "resets")   # the class's counter
I32_MAX = (1 << 31) - 1


def classify(n_lim, permits, limiter, ops, allowed, remaining):
    """(row, class, over_max) of every request; limiter / ops None = limiter 0 / ACQUIRE."""
    n = len(permits)
    lim = np.zeros(n, np.int64) if limiter is None else np.asarray(limiter).astype(np.int64)
    op = np.zeros(n, np.int64) if ops is None else np.asarray(ops).astype(np.int64)
    p = np.asarray(permits).astype(np.int64)
    a = np.asarray(allowed).astype(np.int64)
    r = np.asarray(remaining).astype(np.int64)
    row = np.where(lim < n_lim, lim, rl_amd.TALLY_UNKNOWN)
    cls = np.full(n, -1, np.int64)

    def rule(mask, c):
        cls[(cls < 0) & mask] = c

    rule((lim >= n_lim) | (op > 2) | ((op == rl_amd.OP_ACQUIRE) & (p <= 0)), INVALID)
    rule((a == 0) & (r == rl_amd.REM_ERROR), ERROR)
    rule(op == rl_amd.OP_PEEK, PEEK)
    rule(op == rl_amd.OP_RESET, RESET)
    rule(a != 0, ALLOWED)
    rule(np.ones(n, bool), DENIED)
    over = (cls == DENIED) & (r == rl_amd.REM_UNKNOWN)
    return row, cls, over


def tally_model(n_lim, permits, limiter, ops, allowed, remaining, into=None):
    """rl_tally_batch: a TALLY_DTYPE array of TALLY_ROWS rows (added to `into` if given)."""
    row, cls, over = classify(n_lim, permits, limiter, ops, allowed, remaining)
    out = np.zeros(rl_amd.TALLY_ROWS, rl_amd.TALLY_DTYPE) if into is None else into.copy()
    p = np.asarray(permits).astype(np.int64).astype(np.uint64)     # (only summed where > 0)

    def add(field, mask, weight=None):                               # integer adds, modulo 2^64
        w = np.ones(int(mask.sum()), np.uint64) if weight is None else weight[mask]
        np.add.at(out[field], row[mask], w)

    add("requests", np.ones(len(row), bool))
    for c, f in enumerate(COLS):
        add(f, cls == c)
    add("over_max", over)
    add("permits_allowed", cls == ALLOWED, p)
    add("permits_denied", cls == DENIED, p)
    return out


def top_model(keys, k, min_count):
    """rl_top_keys' definition on a key array: (keys, counts, n_heavy), count descending then key
    ascending unsigned."""
    u, c = np.unique(np.asarray(keys, np.uint64), return_counts=True)
    m = c >= min_count
    u, c = u[m], c[m].astype(np.uint64)
    o = np.lexsort((u, -c.astype(np.int64)))
    return u[o][:k], c[o][:k], int(m.sum())


def top_denied_model(n_lim, keys, permits, limiter, ops, allowed, remaining, sel, k, min_count):
    """rl_top_denied: (keys, counts, n_heavy, n_denied)."""
    row, cls, _ = classify(n_lim, permits, limiter, ops, allowed, remaining)
    s = (row == sel) & (cls == DENIED)
    tk, tc, heavy = top_model(np.asarray(keys, np.uint64)[s], k, min_count)
    return tk, tc, heavy, int(s.sum())


# ---- synthetic batches: results need not be what an engine would answer, only well-formed arrays
MIXES = ("one", "three", "blocks10", "wide")
MIX_LIMITERS = {"one": 1, "three": 3, "blocks10": 10, "wide": 254}


def synth(n, mix, seed=0):
    """(n_lim, permits, limiter, ops, allowed, remaining) of n requests with every sentinel, every
    op (and two that do not exist) and permits up to 2^31 - 1 present whenever n allows."""
    rng = np.random.default_rng(seed * 1000 + n)
    n_lim = MIX_LIMITERS[mix]
    i = np.arange(n)
    if mix == "one":
        lim = np.zeros(n, np.uint16)
    elif mix == "three":
        lim = (i % 3).astype(np.uint16)
    elif mix == "blocks10":
        lim = ((i // 64) % 10).astype(np.uint16)
    else:
        # waves of 64 distinct rows (a stride through the 254 ids), waves of unknown ids
        # 254..65535 that all fall into row 255, and random ones
        lim = ((i * 7) % 254).astype(np.uint16)
        unk = (i // 64) % 3 == 1
        lim[unk] = rng.integers(254, 65536, int(unk.sum())).astype(np.uint16)
        rnd = (i // 64) % 3 == 2
        lim[rnd] = rng.integers(0, 300, int(rnd.sum())).astype(np.uint16)
        if n > 2:
            lim[-1], lim[-2] = 65535, 254
    ops = rng.choice(np.array([0, 0, 0, 0, 0, 1, 2, 3, 255], np.uint8), n)
    permits = rng.choice(np.array([1, 1, 2, 3, 0, -1, I32_MAX, I32_MAX - 1], np.int32), n)
    allowed = rng.choice(np.array([0, 0, 1, 1, 2], np.uint8), n)
    remaining = rng.choice(np.array([0, 5, 7, rl_amd.REM_UNKNOWN, rl_amd.REM_INVALID, rl_amd.REM_ERROR,
                                     -4, 1 << 40], np.int64), n)
    return n_lim, permits, lim, ops, allowed, remaining
