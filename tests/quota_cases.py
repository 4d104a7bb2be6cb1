"""Inputs and oracle-side expectations of tests/test_gpu_quota.py (no GPU, no engine): the
limiters and traces of tests/test_gpu_retry_after.py plus two sparse sliding windows, the query
sets, and the definition of rl_quota evaluated on oracle.rl_oracle.PyOracle by a FULL scan:
  A(t)      = max(0, max - _current_count) for a sliding window, _tb_peek for a token bucket
  remaining = A(now)
  reset     = min{ t in now .. now + 2w + 2 : A(t) == max } - now   (A never drops afterwards)
  retry(p)  = min{ t in now .. now + 2w + ttl + 2 : one acquire of p on a copy of the key's
              state is allowed } - now                               (no denial afterwards)
The scans rely on no monotonicity; they assert it."""
import numpy as np

from oracle.rl_oracle import SW, TB, PyOracle

NS = 1_000_000
T0 = 1_700_000_000_000
NEVER = -1

# (algo, max, window ms, refill/s, cache ttl ms), requests, span ms, trace permits hi, query permits
CASES = [
    ((TB, 5, 1000, 10.0, 0), 1500, 2000, 3, (1, 3, 5, 6)),
    ((TB, 5, 300, 0.5, 0), 600, 1000, 3, (1, 3, 5, 6)),      # expiry before refill
    ((TB, 7, 1000, 3.3, 0), 1500, 2000, 3, (1, 2, 7, 8)),
    ((SW, 10, 200, 0.0, 0), 1500, 500, 2, (1, 4, 10, 11)),
    ((SW, 10, 200, 0.0, 50), 1500, 500, 2, (1, 4, 10, 11)),
    # sparse windows: few enough requests that the window weight, not the PEXPIRE lapse, often
    # decides when the estimate reaches 0
    ((SW, 3, 1000, 0.0, 0), 90, 2500, 1, (1, 2, 3, 4)),
    ((SW, 3, 1000, 0.0, 50), 90, 2500, 1, (1, 2, 3, 4)),
]
N_KEYS = 12                                   # + 1 key that no trace touches


def query_dt(w):
    """Query times, in ms after the trace end."""
    return (0, 1, 37, w)


def mix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def lim_keys(lid):
    return mix64(np.arange(N_KEYS + 1, dtype=np.uint64) + np.uint64((lid + 1) << 32))


def lim_trace(lid):
    """Limiter lid's trace: keys Pareto(1.1)-skewed over its 12 keys, evenly spaced times."""
    _, n, span, pmax, _ = CASES[lid]
    rng = np.random.default_rng(1000 + lid)
    ranks = np.minimum(rng.pareto(1.1, n).astype(np.int64), N_KEYS - 1)
    keys = lim_keys(lid)[ranks]
    permits = rng.integers(1, pmax + 1, n).astype(np.int32)
    now = (T0 * NS + (np.arange(n, dtype=np.int64) * span * NS) // n).astype(np.int64)
    return keys, permits, now, np.full(n, lid, np.uint16)


def trace_end(lid):
    return T0 + CASES[lid][2]


def new_oracle():
    o = PyOracle()
    for (algo, mx, w, rate, ttl), *_ in CASES:
        o.add_limiter(algo, mx, w, rate, local_cache_ttl_ms=ttl)
    for lid in range(len(CASES)):
        o.run(*lim_trace(lid))
    return o


def key_part(o, lid, key):
    """The key's part of the oracle: (redis values, deadlines, cache entries)."""
    pre = (f"{lid}|rl:{key}:", f"{lid}|tb:{key}")
    kv = {k: v for k, v in o.redis.kv.items() if k.startswith(pre[0]) or k == pre[1]}
    exp = {k: o.redis.exp[k] for k in kv if k in o.redis.exp}
    cache = {k: v for k, v in o.cache.items() if k == (lid, key)}
    return kv, exp, cache


def peek(m, L, key, t):
    if L.algo == SW:
        return max(0, L.max_permits - m._current_count(L, key, t))
    return m._tb_peek(L, key, t)[0]


def scan_quota(o, lid, key, permits, now):
    """The definition for one (limiter, key, now): (remaining, reset, [retry(p) for p in permits],
    expiry_decided). expiry_decided: reset > 0 and some live Redis key of this key has its
    PEXPIRE deadline at now + reset - 1 (the quota is back because a key lapsed, not because the
    window weight or the refill got there)."""
    L = o.limiters[lid]
    kv, exp, cache = key_part(o, lid, key)
    m = PyOracle()
    m.limiters = o.limiters
    m.redis.kv, m.redis.exp, m.cache = dict(kv), dict(exp), dict(cache)
    remaining = peek(m, L, key, now)
    reset = None
    for t in range(now, now + 2 * L.window_ms + 2 + 1):
        full = peek(m, L, key, t) == L.max_permits
        if full and reset is None:
            reset = t - now
        assert full or reset is None, ("A drops after first reaching max", lid, key, now, t)
    assert reset is not None, ("no full quota inside the bound", lid, key, now)
    first = {p: None for p in permits}
    for t in range(now, now + 2 * L.window_ms + L.cache_ttl + 2 + 1):
        for p in permits:
            m.redis.kv, m.redis.exp, m.cache = dict(kv), dict(exp), dict(cache)   # the copy
            ok = (m._sw_acquire(L, key, p, t) if L.algo == SW else m._tb_acquire(L, key, p, t))[0]
            if ok and first[p] is None:
                first[p] = t
            assert ok or first[p] is None, ("a denial after the first allow", lid, key, p, now, t)
    retry = []
    for p in permits:
        if p > L.max_permits:
            assert first[p] is None
            retry.append(NEVER)
        else:
            assert first[p] is not None, ("no allow inside the bound", lid, key, p, now)
            retry.append(first[p] - now)
    expiry = reset > 0 and any(d == now + reset - 1 for d in exp.values())
    return remaining, reset, retry, expiry


def query_times(lid):
    return [trace_end(lid) + dt for dt in query_dt(CASES[lid][0][2])]


def build_reference(o):
    """Per limiter a dict of arrays over its 52 (key, time) pairs x its query permits:
    keys, permits, now_ns, limiter, remaining, reset, retry, and per pair (`pair_*`):
    reset, expiry-decided, and retry of p = max (for the identity). Read-only arrays."""
    ref = []
    for lid in range(len(CASES)):
        qp = CASES[lid][4]
        mx = CASES[lid][0][1]
        ps = tuple(qp) + ((mx,) if mx not in qp else ())
        k, p, t, rem, rst, rty = [], [], [], [], [], []
        pair_key, pair_t, pair_reset, pair_exp, pair_retry_max = [], [], [], [], []
        for now in query_times(lid):
            for key in lim_keys(lid):
                r, s, w, e = scan_quota(o, lid, int(key), ps, now)
                pair_key.append(key); pair_t.append(now * NS); pair_reset.append(s); pair_exp.append(e)
                pair_retry_max.append(w[ps.index(mx)])
                for j, pp in enumerate(qp):
                    k.append(key); p.append(pp); t.append(now * NS)
                    rem.append(r); rst.append(s); rty.append(w[j])
        d = dict(keys=np.array(k, np.uint64), permits=np.array(p, np.int32), now_ns=np.array(t, np.int64),
                 limiter=np.full(len(k), lid, np.uint16), remaining=np.array(rem, np.int64),
                 reset=np.array(rst, np.int64), retry=np.array(rty, np.int64),
                 pair_keys=np.array(pair_key, np.uint64), pair_now_ns=np.array(pair_t, np.int64),
                 pair_reset=np.array(pair_reset, np.int64), pair_expiry=np.array(pair_exp, bool),
                 pair_retry_max=np.array(pair_retry_max, np.int64))
        for v in d.values():
            v.setflags(write=False)
        ref.append(d)
    return ref


def check_not_vacuous(ref):
    """The conditions the reference must meet so that equality with it means something; on the
    oracle's answers alone."""
    for lid, d in enumerate(ref):
        r, n = d["pair_reset"], len(d["pair_reset"])
        assert n == 4 * (N_KEYS + 1)
        assert (r > 0).sum() >= 0.25 * n and (r == 0).sum() >= 0.05 * n, (lid, (r > 0).sum(), (r == 0).sum(), n)
        assert (d["retry"] == NEVER).sum() > 0 and (d["retry"] > 0).sum() > 0
    for lid in (3, 5, 6):                                    # SW(10, 200) without cache, the sparse two
        d = ref[lid]
        pos = d["pair_reset"] > 0
        exp, wgt = (pos & d["pair_expiry"]).sum(), (pos & ~d["pair_expiry"]).sum()
        assert exp >= 5 and wgt >= 5, (lid, exp, wgt)

