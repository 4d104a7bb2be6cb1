"""The drivers of the small-batch tests (tests/test_gpu_small_batch.py, tests/test_gpu_small_dirty.py):
a pair of engines, one with rl_tune("small_batch") on and a twin with it off, fed the same
stream, every batch compared bit for bit between the two and against the C oracle."""
import numpy as np

import rl_amd
from oracle.coracle import COracle

MAX = rl_amd.SMALL_BATCH_MAX
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, MAX - 1, MAX)
NS = 1_000_000
T0 = 1_700_000_000_000                      # ms
# rl_batch_stats fields that describe the pipeline's own work (0 after a small batch)
PATH_FIELDS = ("routed", "hot_regions")
GUARD = 7                                   # guard words past n in device outputs
SW = (rl_amd.SW, 5, 1000, 0.0)
TB = (rl_amd.TB, 7, 1000, 3.0)
REM_INVALID, REM_ERROR = -2, -3             # RL_REMAINING_INVALID, RL_REMAINING_ERROR


def words(a):
    return None if a is None else np.ascontiguousarray(a).tobytes()


def same(a, b):
    return words(a) == words(b)


def region_of(keys, slots):
    """The region of each key hash in a table of `slots` slots (include/rl_engine.h: the top bits
    of mix64(key_hash), no shard bits on one engine)."""
    bits = int(slots // rl_amd.REGION_SLOTS).bit_length() - 1
    h = rl_amd.mix64(np.ascontiguousarray(keys, np.uint64))
    return (h >> np.uint64(64 - bits)).astype(np.int64) if bits else np.zeros(len(keys), np.int64)


def keys_of_one_region(count, slots, seed=5):
    rng = np.random.default_rng(seed)
    cand = np.unique(rng.integers(1, 1 << 62, size=count * (slots // rl_amd.REGION_SLOTS) * 4, dtype=np.uint64))
    k = cand[region_of(cand, slots) == 0][:count]
    assert len(k) == count
    return k


class Pair:
    """on: small_batch = `small`; off: the twin; oracle: the C oracle of the same limiters."""

    def __init__(self, lims, small=4 * MAX, oracle=True, max_batch=1 << 12, capacity=1 << 12, **kw):
        self.on = rl_amd.Engine(max_batch=max_batch, capacity=capacity, **kw)
        self.off = rl_amd.Engine(max_batch=max_batch, capacity=capacity, **kw)
        self.oracle = COracle() if oracle else None
        for l in lims:
            spec = dict(zip(("algo", "max_permits", "window_ms", "refill_per_s", "capacity",
                             "local_cache_ttl_ms"), l))
            self.on.add_limiter(**spec)
            self.off.add_limiter(**spec)
            if self.oracle:
                self.oracle.add_limiter(**spec)
        if small is not None:
            self.on.tune("small_batch", small)
        self.taken = self.declined = 0      # what the case expects so far

    def close(self):
        self.on.close()
        self.off.close()

    def expect(self, taken=0, declined=0):
        self.taken += taken
        self.declined += declined
        assert self.on.small_batches() == (self.taken, self.declined)
        assert self.off.small_batches() == (0, 0)

    def _compare(self, got, ref, st_on, st_off, keys, permits, now_ns, limiter, ops, oracle):
        for g, r, name in zip(got, ref, ("allowed", "remaining", "tokens_after")):
            assert same(g, r), f"{name} differs from the twin"
        assert st_on == st_off, (st_on, st_off)
        ls_on, ls_off = self.on.last_status(), self.off.last_status()
        assert ls_on == ls_off == st_on, (ls_on, ls_off, st_on)
        s_on, s_off = self.on.stats(), self.off.stats()
        for f in s_on:
            if f not in PATH_FIELDS:
                assert s_on[f] == s_off[f], (f, s_on[f], s_off[f])
        if oracle and self.oracle:
            oa, orem, ot, _ = self.oracle.run(keys, permits, now_ns, limiter, ops, want_tokens=got[2] is not None)
            assert same(got[0], oa) and same(got[1], orem), "differs from the oracle"
            if got[2] is not None:
                m = ~np.isnan(ot)
                assert same(got[2][m], ot[m]) and np.isnan(got[2][~m]).all()

    def host(self, keys, permits, now_ns, limiter=None, ops=None, want_tokens=True, oracle=True):
        a1, r1, t1, st1 = self.on.execute(keys, permits, now_ns, limiter, ops, want_tokens)
        a0, r0, t0, st0 = self.off.execute(keys, permits, now_ns, limiter, ops, want_tokens)
        self._compare((a1, r1, t1), (a0, r0, t0), st1, st0, keys, permits, now_ns, limiter, ops, oracle)
        return a1, r1, t1, st1

    def device(self, keys, permits, now_ns, limiter=None, ops=None, want_tokens=True, oracle=True,
               stream=None):
        """rl_execute_batch_device on both engines, outputs with sentinel guard words past n."""
        import torch
        n = len(keys)
        dev = torch.device("cuda:0")
        k = torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).to(dev)
        p = torch.from_numpy(np.ascontiguousarray(permits, np.int32)).to(dev)
        t = torch.from_numpy(np.ascontiguousarray(now_ns, np.int64)).to(dev)
        l = None if limiter is None else torch.from_numpy(np.ascontiguousarray(limiter, np.uint16).view(np.int16)).to(dev)
        o = None if ops is None else torch.from_numpy(np.ascontiguousarray(ops, np.uint8)).to(dev)
        out = []
        for e in (self.on, self.off):
            a = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
            r = torch.full((n + GUARD,), -0x1234567, dtype=torch.int64, device=dev)
            tk = torch.full((n + GUARD,), 1.5e300, dtype=torch.float64, device=dev) if want_tokens else None
            torch.cuda.synchronize()
            if stream is not None:
                with torch.cuda.stream(stream):
                    e.execute_device(n, k.data_ptr(), p.data_ptr(), t.data_ptr(),
                                     None if l is None else l.data_ptr(), None if o is None else o.data_ptr(),
                                     a.data_ptr(), r.data_ptr(), None if tk is None else tk.data_ptr(),
                                     stream=stream.cuda_stream)
                stream.synchronize()
            else:
                e.execute_device(n, k.data_ptr(), p.data_ptr(), t.data_ptr(),
                                 None if l is None else l.data_ptr(), None if o is None else o.data_ptr(),
                                 a.data_ptr(), r.data_ptr(), None if tk is None else tk.data_ptr())
            st = e.last_status()
            a, r = a.cpu().numpy(), r.cpu().numpy()
            tk = None if tk is None else tk.cpu().numpy()
            assert (a[n:] == 0xEE).all() and (r[n:] == -0x1234567).all(), "guard words overwritten"
            assert tk is None or (tk[n:] == 1.5e300).all(), "guard words overwritten"
            out.append((a[:n], r[:n], None if tk is None else tk[:n], st))
        (a1, r1, t1, st1), (a0, r0, t0, st0) = out
        self._compare((a1, r1, t1), (a0, r0, t0), st1, st0, keys, permits, now_ns, limiter, ops, oracle)
        return a1, r1, t1, st1

    def digests_equal(self, now_ns, bits=3):
        for lim in range(len(self.on.limiters)):
            d_on, tot_on = self.on.limiter_digest(lim, now_ns, bits)
            d_off, tot_off = self.off.limiter_digest(lim, now_ns, bits)
            assert same(d_on, d_off) and tot_on == tot_off, f"limiter {lim}: digests differ"
            for e in (self.on, self.off):
                rep = e.check_limiter(lim)
                assert rep["bad_slots"] == 0 and not any(rep["violations"]), rep


def mixed_batch(rng, n, n_keys, t_ms, n_lim=2, span_ms=40, permits_max=4):
    keys = rng.integers(1, n_keys + 1, size=n, dtype=np.uint64)
    permits = rng.integers(1, permits_max + 1, size=n, dtype=np.int32)
    now = (t_ms + np.sort(rng.integers(0, span_ms, size=n))).astype(np.int64) * NS
    lim = rng.integers(0, n_lim, size=n, dtype=np.uint16)
    return keys, permits, now, lim


def run_sizes(sizes=SIZES, seed=1, device=False):
    """Every size on one pair, keys drawn from a small universe so that states carry over."""
    P = Pair([SW, TB])
    rng = np.random.default_rng(seed)
    t = T0
    out = []
    for n in sizes:
        k, p, now, lim = mixed_batch(rng, n, 97, t)
        out.append((P.device if device else P.host)(k, p, now, lim))
        P.expect(taken=1)
        t += 173
    # one request more than the path takes: declined, decided by the pipeline
    k, p, now, lim = mixed_batch(rng, MAX + 1, 97, t)
    out.append(P.host(k, p, now, lim))
    P.expect(declined=1)
    P.close()
    return out


def run_one_region(fixed):
    """300 distinct keys of one region of an 8-region table: overflow on a fixed-capacity engine,
    growth on a growing one."""
    P = Pair([SW], oracle=False, capacity=1, fixed_capacity=fixed)
    slots = P.on.limiter_slots(0)
    assert slots == P.off.limiter_slots(0) == 8 * rl_amd.REGION_SLOTS
    k = keys_of_one_region(300, slots)
    n = len(k)
    now = np.full(n, T0 * NS, np.int64)
    a, r, t, st = P.host(k, np.ones(n, np.int32), now, oracle=False)
    P.expect(taken=1)
    if fixed:
        assert st == rl_amd.RL_E_CAPACITY and (r == REM_ERROR).sum() == n - rl_amd.REGION_SLOTS
        assert P.on.limiter_slots(0) == slots
    else:
        assert st == rl_amd.RL_E_CAPACITY or st == rl_amd.RL_OK
        assert P.on.stats()["table_grows"] == P.off.stats()["table_grows"] > 0
        assert P.on.limiter_slots(0) == P.off.limiter_slots(0) > slots
    # the same keys once more (after growth: the region's keys spread over the new regions)
    out = P.host(k, np.ones(n, np.int32), now + 5 * NS, oracle=False)
    P.expect(taken=1)
    assert P.on.limiter_slots(0) == P.off.limiter_slots(0)
    P.close()
    return (a, r, t), out[:3]


def zipf_batch(rng, n, n_keys, t_ms, span_ms=900):
    ranks = np.minimum(rng.zipf(1.2, size=n), n_keys).astype(np.uint64)
    permits = np.ones(n, np.int32)
    now = (t_ms + np.sort(rng.integers(0, span_ms, size=n))).astype(np.int64) * NS
    lim = (ranks % 2).astype(np.uint16)
    return ranks, permits, now, lim


def run_interleaving(n_big=200_000, n_small=50):
    """A large Zipf batch on the pipeline (hot marks, a route list), small batches over the same
    keys, the large batch again: equal digests and clean tables after each phase."""
    P = Pair([(rl_amd.SW, 100, 1000, 0.0), (rl_amd.TB, 50, 1000, 20.0)], small=MAX, oracle=True,
             max_batch=1 << 18, capacity=1 << 14)
    for e in (P.on, P.off):
        e.tune("hot_threshold", 2048)       # the head keys' regions run as hot chains
    rng = np.random.default_rng(9)
    t = T0
    out = [P.host(*zipf_batch(rng, n_big, 5000, t), want_tokens=False)]
    assert P.off.stats()["hot_regions"] > 0
    P.expect()                              # above rl_tune's size: not counted at all
    t += 1000
    P.digests_equal(t * NS)
    for i in range(n_small):
        n = (1, 7, 64, 300, MAX)[i % 5]
        k, p, now, lim = zipf_batch(rng, n, 5000, t, span_ms=30)   # (batches in global time order)
        out.append(P.host(k, p, now, lim))
        P.expect(taken=1)
        t += 37
    P.digests_equal(t * NS)
    out.append(P.host(*zipf_batch(rng, n_big, 5000, t), want_tokens=False))
    P.expect()
    P.digests_equal((t + 1000) * NS)
    P.close()
    return out
