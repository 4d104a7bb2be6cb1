"""One engine over a changing life: the steps and traces of tests/test_gpu_engine_life.py.

Almost every GPU test builds a fresh engine per case and feeds it batches of one shape under one
set of knobs. A service's engine lives for days: it meets a small batch after a large one, a wide
one after a compact one, the hot path switched off and on, a table that crosses from one partition
pass to two and back, and every such change leaves stale words behind in buffers that are reused
(DESIGN §7a lists them). Each case here is ONE engine and ONE continuing trace (time only moves
forward, state persists); every batch is checked on its own against the oracle.

A case is a list of steps:
    ("tune", key, value)                      rl_tune between two batches
    ("batch", Batch)                          one batch; Batch.hot / Batch.routed say which path must
                                              have run (None: not asserted)
    ("grow", limiter, min_keys)               rl_grow_limiter
    ("shrink", limiter, min_keys)             rl_shrink_limiter at the last batch's end
    ("add_limiter", spec)                     a further limiter (engine and oracle)
    ("width", w)                              rl_result_width must be w here
    ("regions", "one" | "two")                the partition passes the table's region count implies

Plain numpy, no GPU: tests/test_life_cases_model.py checks with the oracle alone that every batch
of every case is meaningful (it allows and denies; a hot batch has a region at the threshold, a
"none" batch has none)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import rl_amd

NS = 1_000_000
T0 = 1_700_000_000_000
SW, TB = rl_amd.SW, rl_amd.TB
TILE = 4096                                  # requests per partition tile at tile_items = 8
ONE_PASS = 1 << 14                           # keys of the whole table: 2 x 64 regions, one pass
TWO_PASS = 1 << 21                           # 2 x 8,192 regions: region ids of 14 bits, two passes
MAX_ONE_PASS_REGIONS = 8192                  # 2^kMaxDigitBits (csrc/rl_device.hpp)
LIMS = [[SW, 3, 2_000, 0.0], [TB, 5, 2_000, 1.0]]
HOT_THR = 256
BAD_LIMITER = 7
SPAN_MS = 1_000                              # a batch's time slice


def hot_set(tag, n=3):
    return rl_amd.mix64(np.arange(n, dtype=np.uint64) + np.uint64(tag << 40))


X, Y = hot_set(0xA1), hot_set(0xA2)
# A named key always comes under the same limiter, whatever list it arrives in: its region must
# not move between the batch that makes it hot and the next one.
KEY_LIMITER = {int(k): j % 2 for s in (X, Y) for j, k in enumerate(s)}


def limiter_of(key):
    return KEY_LIMITER.get(int(key), 0)


@dataclass
class Batch:
    tr: tuple                                # keys, permits, now_ns, limiter, op
    want_tokens: bool = True
    entry: str = "host"                      # "host": rl_execute_batch; "device": caller tensors of n
    hot: object = None                       # True: hot_regions >= 1; False: == 0
    routed: object = None                    # True: routed > 0; False: == 0
    cache_hits: object = None                # True: cache_hits > 0
    hot_keys: object = None                  # the model test's: keys that make a region hot / None
    none: bool = False                       # the model test's: no region reaches the threshold
    note: str = ""


@dataclass
class Case:
    name: str
    capacity: int                            # keys of the whole table, split evenly over `limiters`
    steps: list
    limiters: list = field(default_factory=lambda: [list(l) for l in LIMS])
    tune: dict = field(default_factory=dict)  # before the first batch
    tile_items: int = 8                      # 0: the engine's default tiles
    max_batch: int = 1 << 17
    pipeline: bool = False                   # RL_OPT_PIPELINE, device entry, no sync between calls
    hot_thr: int = HOT_THR

    def batches(self):
        return [s[1] for s in self.steps if s[0] == "batch"]


# ---------------------------------------------------------------- regions (the model test)
def region_bits(capacity_keys):
    """Region bits of a limiter added with room for capacity_keys (rl_add_limiter_ex: load 0.5,
    whole bins of MIN_REGIONS regions)."""
    slots = max(2 * capacity_keys, rl_amd.REGION_SLOTS)
    regions = -(-slots // rl_amd.REGION_SLOTS)
    return max((regions - 1).bit_length(), rl_amd.MIN_REGIONS.bit_length() - 1)


def grown_bits(bits, min_keys):
    """rl_grow_limiter: doubled until the table holds 2 x min_keys slots."""
    while (rl_amd.REGION_SLOTS << bits) < 2 * min_keys:
        bits += 1
    return bits


def region_counts(tr, bits_per_limiter):
    """Records per (limiter, region) of a batch, as test_capacity_overflow_reported computes a
    key's region: the top region bits of mix64(key). Unknown limiter ids go to limiter 0."""
    keys, lim = tr[0], tr[3].astype(np.int64)
    lim = np.where(lim < len(bits_per_limiter), lim, 0)
    h = rl_amd.mix64(keys)
    out = []
    for l, bits in enumerate(bits_per_limiter):
        m = lim == l
        region = (h[m] >> np.uint64(64 - bits)).astype(np.int64)
        out.append(np.bincount(region, minlength=1 << bits))
    return out


# ---------------------------------------------------------------- traffic
def traffic(seed, n_bg, t_ms, hot=(), hot_each=0, cool=(), cool_each=0, n_keys=4000, n_lim=2,
            span_ms=SPAN_MS, permits_max=2, ops=0.01, tag=0xB1):
    """n_bg requests over n_keys uniform background keys, hot_each requests of every key of `hot`
    and cool_each of every key of `cool` (each under its own fixed limiter, limiter_of), in
    [t_ms, t_ms + span_ms), in arrival order."""
    rng = np.random.default_rng(seed)
    ranks = rng.integers(0, n_keys, n_bg)
    keys = [rl_amd.mix64(ranks.astype(np.uint64) + np.uint64(tag << 40))]
    lim = [(ranks % n_lim).astype(np.uint16)]
    for ks, each in ((hot, hot_each), (cool, cool_each)):
        for k in ks:
            keys.append(np.full(each, k, np.uint64))
            lim.append(np.full(each, limiter_of(k), np.uint16))
    keys, lim = np.concatenate(keys), np.concatenate(lim)
    n = len(keys)
    ms = rng.integers(0, span_ms, n)
    o = np.argsort(ms, kind="stable")
    permits = rng.integers(1, permits_max + 1, n).astype(np.int32)
    op = np.zeros(n, np.uint8)
    u = rng.random(n)
    op[u < ops] = rl_amd.OP_PEEK
    op[u < ops / 2] = rl_amd.OP_RESET
    return keys[o], permits, ((t_ms + ms[o]) * NS).astype(np.int64), lim[o], op


def shapes_traffic(seed, n, t_ms, span_ms=SPAN_MS, n_keys=3000, n_lim=2):
    """n requests over mildly skewed keys with about 1 % peeks and resets and 0.5 % each of unknown
    limiter ids, unknown operations and zero permits (test_gpu_partition_shapes.shape_trace's mix)
    in [t_ms, t_ms + span_ms)."""
    rng = np.random.default_rng(seed)
    ranks = np.minimum(rng.zipf(1.2, n), n_keys) - 1
    keys = rl_amd.mix64(ranks.astype(np.uint64) + np.uint64(0xB2 << 40))
    lim = (ranks % n_lim).astype(np.uint16)
    now = ((t_ms + np.sort(rng.integers(0, span_ms, n))) * NS).astype(np.int64)
    permits = rng.integers(1, 3, n).astype(np.int32)
    op = np.zeros(n, np.uint8)
    u = rng.random(n)
    op[u < 0.01] = rl_amd.OP_PEEK
    op[u < 0.005] = rl_amd.OP_RESET
    v = rng.random(n)
    lim[v < 0.005] = BAD_LIMITER
    op[(v >= 0.005) & (v < 0.010)] = 9
    permits[(v >= 0.010) & (v < 0.015)] = 0
    return keys, permits, now, lim, op


def hot_batch(seed, i, hotset, n_bg=4096, cool_each=60, **kw):
    """Batch i of a hot case: `hotset` (X, Y or None) draws 600 requests per key, the other set's
    keys a sub-threshold trickle, so a region hot in one batch is a normal one in the next."""
    hot = () if hotset is None else hotset
    mine = set() if hotset is None else {int(k) for k in hotset}
    cool = [k for s in (X, Y) for k in s if int(k) not in mine]
    tr = traffic(seed * 100 + i, n_bg, T0 + i * SPAN_MS, hot=hot, hot_each=600, cool=cool,
                 cool_each=cool_each)
    return Batch(tr, want_tokens=i % 2 == 0, hot_keys=None if hotset is None else hotset,
                 none=hotset is None, **kw)


# ---------------------------------------------------------------- 1. sizes falling and rising
SIZES = (65_536 + 513, 1, 4_097, 63, 3 * TILE + 513, 64, 65, 65_536 + 513)


def case_sizes(split, entry="host"):
    steps = []
    for i, n in enumerate(SIZES):
        tr = shapes_traffic(1100 + i, n, T0 + i * SPAN_MS)
        steps.append(("batch", Batch(tr, want_tokens=i % 2 == 0, entry=entry, note=f"n={n}")))
    return Case(f"sizes-split{split}-{entry}", ONE_PASS, steps,
                tune=dict(scatter_split=split, unpermute_split=split))


# ---------------------------------------------------------------- 2. the hot path comes and goes
HOT_PATTERN = (X, Y, None, X, X, Y, None, X, X, Y, None, X)
HOT_KNOBS = {1: ("hot_threshold", 0), 2: ("hot_threshold", HOT_THR), 3: ("walk", 0), 4: ("walk", 1),
             5: ("chain_split", 0), 6: ("route", 0), 7: ("route", 1), 8: ("segments", 4),
             9: ("segments", 1), 10: ("region_order", 0)}


def case_hot(two_pass):
    steps = []
    thr, route, table = HOT_THR, 1, None      # `table`: the hot set whose regions the route table lists
    for i, hs in enumerate(HOT_PATTERN):
        if i in HOT_KNOBS:
            k, v = HOT_KNOBS[i]
            steps.append(("tune", k, v))
            thr = v if k == "hot_threshold" else thr
            route = v if k == "route" else route
        routes = bool(two_pass and thr and route)
        # (a routed region goes through the chains whatever its size: it counts as a hot region)
        hot = bool(thr) and (hs is not None or (routes and table is not None))
        routed = (routes and table is not None) if two_pass else None
        steps.append(("batch", hot_batch(21, i, hs, hot=hot, routed=routed)))
        if routes:
            table = hs                         # k_route_next rebuilds the table from this batch's hot list
    return Case("hot-two-pass" if two_pass else "hot-one-pass", TWO_PASS if two_pass else ONE_PASS,
                steps, tune=dict(hot_threshold=HOT_THR, walk_min=0))


# ---------------------------------------------------------------- 3. the epoch wraps
def case_epoch(pipeline):
    b = [hot_batch(31, 0, X, hot=True), hot_batch(31, 1, Y, hot=True),
         hot_batch(31, 2, Y, hot=True, cool_each=150), hot_batch(31, 3, X, hot=True)]
    if pipeline:
        for x in b:
            x.entry = "device"
    steps = [("batch", b[0]), ("tune", "hot_epoch", 0xFFFFFFFE), ("batch", b[1]), ("batch", b[2]),
             ("batch", b[3])]
    return Case("epoch-pipelined" if pipeline else "epoch", ONE_PASS, steps,
                tune=dict(hot_threshold=HOT_THR), pipeline=pipeline)


# ---------------------------------------------------------------- 4. the pass count crosses over
def case_passes():
    third = [SW, 4, 1_500, 0.0]
    steps = [("regions", "one")]
    for i in range(2):
        steps.append(("batch", hot_batch(41, i, X, hot=True)))
    steps += [("grow", 0, 1 << 20), ("regions", "two")]
    for i in range(2, 5):
        steps.append(("batch", hot_batch(41, i, X, hot=True, routed=True if i > 2 else None)))
    steps += [("shrink", 0, 1 << 13), ("regions", "one")]
    for i in range(5, 7):
        steps.append(("batch", hot_batch(41, i, X if i == 5 else Y, hot=True)))
    steps.append(("add_limiter", third))
    tr = traffic(4107, 6000, T0 + 7 * SPAN_MS, hot=X, hot_each=600, n_lim=3)
    steps.append(("batch", Batch(tr, hot=True, hot_keys=X)))
    return Case("passes", ONE_PASS, steps, tune=dict(hot_threshold=HOT_THR), max_batch=1 << 17)


# ---------------------------------------------------------------- 5. compact, wide, compact
WIDTH_LIMS = [[SW, 124, 60_000, 0.0], [TB, 124, 60_000, 1000.0]]   # test_gpu_result_widths' edge: 1 byte
WIDTH_4 = [TB, 32_765, 60_000, 1000.0]                               # the first 4-byte maximum
WIDTH_8 = [TB, 4_194_303, 60_000, 1000.0]                            # the first wide-record maximum


def width_traffic(seed, n, i, n_lim=2, far=0):
    """Few keys, so that the sliding window's busiest pass 124 per minute; `far` extra token-bucket
    requests on keys of their own 2^33 ms later (a batch no compact record holds)."""
    tr = traffic(seed + i, n, T0 + i * SPAN_MS, n_keys=40, n_lim=n_lim, permits_max=3, ops=0.02, tag=0xB5)
    if not far:
        return tr
    k = rl_amd.mix64(np.arange(far, dtype=np.uint64) + np.uint64(0xB6 << 40))
    at = np.linspace(10, n - 10, far).astype(int)
    keys, permits, now, lim, op = (x.copy() for x in tr)
    keys[at], permits[at], lim[at], op[at] = k, 2, 1, 0
    now[at] = (T0 + i * SPAN_MS + (1 << 33)) * NS
    return keys, permits, now, lim, op


def case_widths():
    mk = lambda n, i, **kw: Batch(width_traffic(5100, n, i, **kw), want_tokens=i % 2 == 0)  # noqa: E731
    far = mk(3_000, 3, far=6)
    far.note = "spans more than 2^32 ms: the host entry's retry in wide records"
    steps = [("width", 1), ("batch", mk(20_000, 0)), ("tune", "wide_records", 1),
             ("batch", mk(5_000, 1)), ("tune", "wide_records", 0), ("batch", mk(9_000, 2)),
             ("batch", far), ("batch", mk(4_097, 4)), ("width", 1),
             ("add_limiter", WIDTH_4), ("width", 4), ("batch", mk(6_000, 5, n_lim=3)),
             ("add_limiter", WIDTH_8), ("width", 8), ("batch", mk(2_000, 6, n_lim=4)),
             ("batch", mk(8_000, 7, n_lim=4))]
    return Case("widths", ONE_PASS, steps, limiters=[list(l) for l in WIDTH_LIMS])


# ---------------------------------------------------------------- 6. scratch regrowth
REGROW_SIZES = ((1 << 20) + 5_000, 1_300_000, 5_000)


def case_regrow(middle_wide):
    steps = []
    for i, n in enumerate(REGROW_SIZES):
        if middle_wide and i in (1, 2):
            steps.append(("tune", "wide_records", 1 if i == 1 else 0))
        tr = shapes_traffic(6100 + i, n, T0 + i * SPAN_MS, n_keys=200_000)
        steps.append(("batch", Batch(tr, want_tokens=i == 1, note=f"n={n}")))
    return Case("regrow-wide" if middle_wide else "regrow", 1 << 19, steps, tile_items=0,
                max_batch=1 << 21)


# ---------------------------------------------------------------- 7. pipelined sets of different ages
PIPE_SIZES = (20_000, 800, 20_000, 800, 800, 20_000, 800)


def case_pipeline():
    steps = []
    for i, n in enumerate(PIPE_SIZES):
        b = hot_batch(71, i, X, n_bg=n, hot=None)
        b.entry, b.want_tokens = "device", False
        steps.append(("batch", b))
    last = steps[-1][1]
    last.hot, last.routed = True, True
    return Case("pipeline", TWO_PASS, steps, tune=dict(hot_threshold=HOT_THR), pipeline=True)


# ---------------------------------------------------------------- 8. cache-on limiters, the solo pass
CACHE_LIMS = [[SW, 10, 1_000, 0.0, 0, 50], [TB, 5, 2_000, 1.0]]


def case_solo():
    steps = []
    hot = hot_set(0xA8, 1)                    # one key of the cache-on limiter (limiter 0), at its limit
    for i, thr in enumerate((4096, 64, 0, 64, 64)):
        steps.append(("tune", "solo_threshold", thr))
        tr = traffic(8100 + i, 5_000 if i != 4 else 900, T0 + i * SPAN_MS, hot=hot, hot_each=1500 if i != 4 else 300)
        steps.append(("batch", Batch(tr, want_tokens=i % 2 == 0, cache_hits=True,
                                     note=f"solo_threshold={thr}")))
    return Case("solo", ONE_PASS, steps, limiters=[list(l) for l in CACHE_LIMS])


# ---------------------------------------------------------------- the cases
CASES = {
    "sizes-split0": lambda: case_sizes(0),
    "sizes-split1": lambda: case_sizes(1),
    "sizes-device": lambda: case_sizes(1, entry="device"),
    "hot-one-pass": lambda: case_hot(False),
    "hot-two-pass": lambda: case_hot(True),
    "epoch": lambda: case_epoch(False),
    "epoch-pipelined": lambda: case_epoch(True),
    "passes": case_passes,
    "widths": case_widths,
    "regrow": lambda: case_regrow(False),
    "regrow-wide": lambda: case_regrow(True),
    "pipeline": case_pipeline,
    "solo": case_solo,
}


@functools.lru_cache(maxsize=None)
def get(name):
    """The case and, per batch, what the oracle decides (computed once, shared, read-only)."""
    from oracle.coracle import COracle
    case = CASES[name]()
    o = COracle(case.limiters)
    want = []
    for s in case.steps:
        if s[0] == "add_limiter":
            o.add_limiter(*s[1])
        elif s[0] == "batch":
            w = o.run(*s[1].tr)
            for x in tuple(s[1].tr) + w[:3]:
                x.setflags(write=False)
            want.append(w + (o.cache_hits(),))
    o.close()
    return case, want
