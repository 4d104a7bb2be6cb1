"""The inputs of tests/test_gpu_route_kernels.py, in one place so that tests/test_route_model.py
checks on the CPU, from route_model alone, that every set has the properties the GPU tests rely
on: each adversarial owner pattern really produces the owners it claims, each escape case really
holds the stated number of escapes per segment, the wire edges sit where they say."""
import numpy as np

import rl_amd
import route_model as rm

NS = rm.NS
T0_MS = 1_700_000_000_000
TILE = 65536                                       # requests per partition tile (kTile)
SENT = 0xA5                                        # pre-fill byte of every output
GUARD = 64                                         # bytes after every output that must survive

SIZES = [0, 1, 255, 256, 257, 5000]                # one-block edges of the 256-thread kernels
WIDTHS = [1, 2, 4, 8]

# ---------------------------------------------------------------- owner partition
PART_N = 2 * TILE + 777                            # two full tiles and a ragged one
PART_SHARDS = [2, 16, 64]
PATTERNS = ["one", "round_robin", "runs", "descending", "absent"]
RUN_SWITCH = 37                                    # runs switch owner at index = 37 mod 64: mid-wave


def pattern_owners(pattern, shards, n=PART_N):
    """The owner every request of an adversarial batch is meant to have."""
    i = np.arange(n, dtype=np.int64)
    if pattern == "one":                           # 64-way matches in every wave
        return np.full(n, (shards - 1) // 2, np.uint32)
    if pattern == "round_robin":                   # at 64 shards every lane of a wave differs
        return (i % shards).astype(np.uint32)
    if pattern == "runs":                          # runs of 64 that switch inside a wave
        return (((i + 64 - RUN_SWITCH) // 64) % shards).astype(np.uint32)
    if pattern == "descending":
        return (shards - 1 - i * shards // n).astype(np.uint32)
    if pattern == "absent":                        # owner 0 receives nothing
        rng = np.random.default_rng(1000 + shards)
        return rng.integers(1, shards, n).astype(np.uint32)
    raise ValueError(pattern)


_pools = {}


def owner_pools(shards):
    """Per-owner pools of key hashes: random u64 bucketed by the model's owners."""
    if shards not in _pools:
        rng = np.random.default_rng(77 + shards)
        k = rng.integers(0, 2 ** 64, 256 * shards, dtype=np.uint64)
        own = rm.owners(k, shards)
        _pools[shards] = [k[own == s] for s in range(shards)]
    return _pools[shards]


def pattern_keys(pattern, shards, n=PART_N):
    want = pattern_owners(pattern, shards, n)
    pools = owner_pools(shards)
    keys = np.zeros(n, np.uint64)
    for s in range(shards):
        idx = np.nonzero(want == s)[0]
        keys[idx] = pools[s][np.arange(idx.size) % pools[s].size]
    return keys


def skip_mask(pattern, shards, n=PART_N):
    """A 50 % skip mask (non-zero bytes of several values skip)."""
    rng = np.random.default_rng(PATTERNS.index(pattern) * 100 + shards)
    return (rng.random(n) < 0.5).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)


# the full directory: kDirMax keys at 64 shards
DIR_MAX = 4096
DIR_SHARDS = 64
DIR_BATCH = 70_000


def full_directory(n=DIR_MAX, shards=DIR_SHARDS):
    keys = rl_amd.mix64(np.arange(n, dtype=np.uint64) + np.uint64(0xD1C7))
    return keys, ((3 + 7 * np.arange(n)) % shards).astype(np.uint32)


def directory_batch():
    """DIR_BATCH requests, half of them on the directory's keys."""
    dk, _ = full_directory()
    rng = np.random.default_rng(4096)
    keys = rng.integers(0, 2 ** 64, DIR_BATCH, dtype=np.uint64)
    hit = np.arange(DIR_BATCH) % 2 == 0
    keys[hit] = dk[rng.integers(0, DIR_MAX, int(hit.sum()))]
    return keys, hit


def other_keys(n=1000):
    return np.random.default_rng(4097).integers(0, 2 ** 64, n, dtype=np.uint64)


# ---------------------------------------------------------------- pack / fold / unpack
def request_arrays(n, seed=0):
    """(perm, keys, permits, now_ns, limiter) of n requests; permits of either sign."""
    rng = np.random.default_rng(9000 + 31 * n + seed)
    return (rng.permutation(n).astype(np.uint32),
            rng.integers(0, 2 ** 64, n, dtype=np.uint64),
            rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32),
            (T0_MS * NS + rng.integers(-10_000 * NS, 10_000 * NS, n)).astype(np.int64),
            rng.integers(0, 2 ** 16, n).astype(np.uint16))


FOLD_REMAINING = [-2 ** 62, -5000, -4, -3, -2, -1, 0, 1, 124, 2 ** 62 - 1]
FOLD_ALLOWED = [0, 1, 0xFF]                        # only bit 0 counts


def fold_case(n):
    """(allowed, remaining) cycling through every pair of FOLD_ALLOWED x FOLD_REMAINING."""
    pairs = np.array([(a, r) for a in FOLD_ALLOWED for r in FOLD_REMAINING], np.int64)
    pick = np.random.default_rng(n).permutation(n) % len(pairs)
    return pairs[pick, 0].astype(np.uint8), pairs[pick, 1].copy()


def packed_case(n, w):
    """(allowed, remaining) inside the documented domain of rl_route_fold_packed at width w:
    remaining in [-3, width_hi(w)] with both ends, -1, -2, -3 and random interior values,
    without the pair (allowed 1, remaining -3)."""
    rng = np.random.default_rng(100 * n + w)
    hi = rm.width_hi(w)
    r = rng.integers(-3, min(hi, 2 ** 62) + 1, n).astype(np.int64)
    fixed = np.array([-3, hi, -1, -2, hi - 1, 0], np.int64)
    where = rng.permutation(n)[:len(fixed)]
    r[where] = fixed[:where.size]
    a = rng.integers(0, 2, n).astype(np.uint8) * rng.choice(np.array([1, 0xFF], np.uint8), n)
    a[r == -3] = 0
    return a, r


# ---------------------------------------------------------------- segmented return trip
RET_N = 4501                                       # > 4096 + 5; RET_N * w is no multiple of 8 for w < 8
SEG_LISTS = {
    "one": [RET_N],
    "empty_first": [0, RET_N],
    "empty_last": [RET_N, 0],
    "small": [3, 0, 0, 5, 1],
    "sixty_four": [(37 * i) % 11 for i in range(64)],
    "residues": [1, 2, 3, 4, 5, 6, 7, 8],          # count * w mod 8: every residue w allows
}
EXC_CAPS = [0, 1, 4, 4096]
ESC_KINDS = ["none", "cap", "cap_plus_1", "cap_plus_5"]


def escape_targets(seg_counts, cap, kind):
    """Escapes per segment: 0, exactly cap, cap + 1 or cap + 5, as far as the segment has requests."""
    want = {"none": 0, "cap": cap, "cap_plus_1": cap + 1, "cap_plus_5": cap + 5}[kind]
    return [min(want, int(c)) for c in seg_counts]


def return_case(name, w, cap, kind):
    """(seg_counts, allowed, remaining, perm) with exactly escape_targets escapes per segment.
    An escape is a remaining below -3, or (w < 8) above width_hi(w) with allowed 0. A segment
    with two or more escapes has them at its first and its last position; with one, at the
    first (even segments) or the last (odd segments)."""
    counts = SEG_LISTS[name]
    n = sum(counts)
    rng = np.random.default_rng(list(SEG_LISTS).index(name) * 1000 + w * 100 + EXC_CAPS.index(cap) * 10
                                + ESC_KINDS.index(kind))
    a, r = packed_case(n, w) if n else (np.zeros(0, np.uint8), np.zeros(0, np.int64))
    a, r = a.copy(), r.copy()
    hi = rm.width_hi(w)
    low = np.array([-4, -5, -5000, -2 ** 62, -2 ** 63], np.int64)
    high = np.array([hi + 1, hi + 2, 2 ** 62 - 1 if hi < 2 ** 62 - 1 else hi + 3], np.int64) if w < 8 else low
    beg = 0
    for s, (c, k) in enumerate(zip(counts, escape_targets(counts, cap, kind))):
        if k:
            pos = [0, c - 1] if k >= 2 else [0 if s % 2 == 0 else c - 1]
            rest = np.setdiff1d(np.arange(c), pos)
            pos = np.array(pos + rng.permutation(rest)[:k - len(pos)].tolist(), np.int64)[:k]
            up = rng.random(pos.size) < 0.4
            r[beg + pos] = np.where(up, high[rng.integers(0, len(high), pos.size)],
                                    low[rng.integers(0, len(low), pos.size)])
            a[beg + pos] = np.where(r[beg + pos] > hi, 0, a[beg + pos])
        beg += c
    return list(counts), a, r, rng.permutation(n).astype(np.uint32)


# ---------------------------------------------------------------- compact wire
WIRE_BLOCKS_MAX = 2048                             # kWireBlocksMax blocks of 256 requests, then a stride
WIRE_BIG = WIRE_BLOCKS_MAX * 256 + 321
WIRE_SIZES = [0, 1, 257, WIRE_BIG]
WIRE_EPOCHS = {"t0": T0_MS * NS + 123_456, "epoch": -1_500_001}     # now_ns of request 0
# (offset in ms of one request from request 0's ms, overflow flag)
WIRE_EDGES = [(-2 ** 31, 0), (-2 ** 31 - 1, 1), (2 ** 31 - 1, 0), (2 ** 31, 1)]


def wire_case(n, epoch):
    """(perm, keys, permits, now_ns, limiter): times within 10 s of WIRE_EPOCHS[epoch], so at
    "epoch" about half of them are negative and none is a whole millisecond by construction."""
    perm, keys, permits, _, lim = request_arrays(n, seed=1)
    rng = np.random.default_rng(n + len(epoch))
    now = (WIRE_EPOCHS[epoch] + rng.integers(-10_000, 10_000, n) * NS).astype(np.int64)
    if n:
        now[0] = WIRE_EPOCHS[epoch]
    return perm, keys, permits, now, lim


def wire_edge_case(n, epoch, offset_ms, last_stride):
    """wire_case with one request (not request 0) moved offset_ms from request 0's ms. With
    last_stride its place in owner order is past the first WIRE_BLOCKS_MAX * 256 requests."""
    perm, keys, permits, now, lim = wire_case(n, epoch)
    j = n - 5 if last_stride else n // 2
    i = int(perm[j])
    if i == 0:
        j -= 1
        i = int(perm[j])
    ms0 = int(np.floor_divide(now[0], NS))
    now = now.copy()
    now[i] = (ms0 + offset_ms) * NS + 999_999      # the last nanosecond of that ms
    return perm, keys, permits, now, lim, j


UNWIRE_COUNTS = [(37 * i) % 11 for i in range(64)]             # several empty sources
UNWIRE_BASES = [(-1) ** i * (T0_MS // 3) * (i % 5) + 1_000_003 * i - 2 ** 31 for i in range(64)]


def unwire_case():
    m = sum(UNWIRE_COUNTS)
    rng = np.random.default_rng(6464)
    return rng.integers(0, 2 ** 64, (m, 2), dtype=np.uint64)


# ---------------------------------------------------------------- ops column
OPS_LIMITERS = [0, 1, 254, 255, 0x3FFE, 0x3FFF, 0x4000, 0x4001, 0xFFFF]
OPS_OPS = [0, 1, 2, 3, 255]


def ops_case(n):
    pairs = np.array([(l, o) for l in OPS_LIMITERS for o in OPS_OPS], np.uint32)
    rng = np.random.default_rng(n + 3)
    pick = rng.permutation(n) % len(pairs)
    return rng.permutation(n).astype(np.uint32), pairs[pick, 0].astype(np.uint16), pairs[pick, 1].astype(np.uint8)
