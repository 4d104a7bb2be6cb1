"""The rules of the table check (csrc/rl_check.hpp, rl_check_limiter in include/rl_engine.h)
restated in plain Python, slot by slot: this is the definition the kernel is compared with. Also a
placement model that builds healthy synthetic tables (mix64, region_local, slot_home, linear
probing, tombstones left in place) and one corruption per class with the count and the first
position it must produce.

A table is `Table`: slots[R, 256, 4] uint64 = {tag, a, b, c} and, with a cache table, cache[R, 256].
The engine's shard bits are 0 in every case here (one shard)."""
import numpy as np

M64 = (1 << 64) - 1
NS = 256
NONE = M64
CLASSES = 16
(WRONG_REGION, UNREACHABLE, DUPLICATE, DEAD_MARK, SW_START, SW_COUNT, SW_OFFSET, TB_FLAGS, TB_TOKENS,
 IMAGE_LIMITER, IMAGE_RESERVED) = range(11)
DEAD = 2                                    # kDeadMark
SW, TB = 0, 1
W = 4000                                    # window_ms of every limiter here
T0 = 1_700_000_000_000                      # a multiple of W
MAXP = 6
BITS = 3                                    # 8 regions


def mix64(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def region_local(tag, shard_bits, k):
    return ((tag << shard_bits) & M64) >> (64 - k) if k else 0


def slot_home(tag):
    return tag & (NS - 4)


def i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def i64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def trunc_mod(a, w):
    """C's a % w for w > 0 (the sign of a)."""
    return a % w if a >= 0 else -((-a) % w)


# ---------------------------------------------------------------------------- the definition
def holds_state(algo, b, c, x):
    return x != 0 or ((c & 1) != 0 if algo == TB else b != 0)


def slot_values(algo, w, tag, a, b, c, x):
    """Class ids of one used slot that need its words only (DEAD_MARK and the value classes)."""
    out = set()
    if algo == TB:
        if c == DEAD:
            if tag or a or b or x:
                out.add(DEAD_MARK)
        elif c & ~1:
            out.add(TB_FLAGS)
        return out
    c1, c0 = b & 0xFFFFFFFF, b >> 32
    o1, o0 = i32(c), i32(c >> 32)
    if b != 0 and trunc_mod(i64(a), w) != 0:
        out.add(SW_START)
    if (c1 and not -w < o1 < w) or (c0 and not -w < o0 < w):
        out.add(SW_OFFSET)
    return out


def last_write(algo, w, a, b, c):
    """When a slot's bucket state was last written (None: it holds none). TB: the last refill; SW:
    the newest last-INCR time of its buckets with a count. 64-bit wrapping, as the kernel computes."""
    if algo == TB:
        return i64(b) if c & 1 else None
    if b == 0:
        return None
    c1, c0 = b & 0xFFFFFFFF, b >> 32
    t1, t0 = i64(a + i32(c)), i64(a - w + i32(c >> 32))
    return t1 if c1 and (not c0 or t1 >= t0) else t0


def copies_conflict(x, y, ttl):
    """Two copies of a tag both claim the key unless one had expired before the other's last write
    (the stale slot a returning key leaves behind when it claims an earlier tombstone)."""
    return not (x + ttl < y) and not (y + ttl < x)


def empty_report(regions, slots):
    return dict(regions=regions, slots=slots, used_slots=0, state_slots=0, tombstones=0, cache_words=0,
                bad_slots=0, violations=[0] * CLASSES, first=[NONE] * CLASSES)


def _count(rep, classes, pos):
    if classes:
        rep["bad_slots"] += 1
    for c in classes:
        rep["violations"][c] += 1
        rep["first"][c] = min(rep["first"][c], pos)


def check_model(t, algo, w=W, shard_bits=0, region_begin=0, region_count=1 << 62):
    """rl_check_limiter / rl_check_table_device over regions [region_begin, +region_count) of t."""
    R = t.slots.shape[0]
    k = R.bit_length() - 1
    lo = min(region_begin, R)
    hi = min(R, lo + region_count)
    rep = empty_report(hi - lo, (hi - lo) * NS)
    for r in range(lo, hi):
        rows = [tuple(int(v) for v in t.slots[r, s]) + (int(t.cache[r, s]) if t.cache is not None else 0,)
                for s in range(NS)]
        used = [any(row) for row in rows]
        seen = {}                            # tag -> last writes of its copies at lower indices
        ttl = 2 * w if algo == TB else w
        for s, (tag, a, b, c, x) in enumerate(rows):
            rep["cache_words"] += x != 0
            if not used[s]:
                continue
            rep["used_slots"] += 1
            if holds_state(algo, b, c, x):
                rep["state_slots"] += 1
            else:
                rep["tombstones"] += 1
            cls = slot_values(algo, w, tag, a, b, c, x)
            if region_local(tag, shard_bits, k) != r:
                cls.add(WRONG_REGION)
            p = slot_home(tag)
            while p != s:                    # the probe, slot by slot
                if not used[p]:
                    cls.add(UNREACHABLE)
                    break
                p = (p + 1) % NS
            lw = last_write(algo, w, a, b, c)
            if lw is not None and any(o is not None and copies_conflict(lw, o, ttl) for o in seen.get(tag, ())):
                cls.add(DUPLICATE)
            seen.setdefault(tag, []).append(lw)
            _count(rep, cls, r << 8 | s)
    return rep


def check_images_model(images, lims):
    """rl_check_images: `lims` = [(algo, window_ms)] of the engine, images a KEY_IMAGE_DTYPE array."""
    rep = empty_report(0, len(images))
    for i, im in enumerate(images):
        tag = mix64(int(im["key_hash"]))
        a, b, c = (int(v) for v in im["word"])
        x, lim = int(im["cache_word"]), int(im["limiter"])
        used = bool(tag or a or b or c or x)
        rep["cache_words"] += x != 0
        rep["used_slots"] += used
        cls = set()
        if any(int(v) for v in im["reserved"]):
            cls.add(IMAGE_RESERVED)
        state = False
        if lim >= len(lims):
            cls.add(IMAGE_LIMITER)
        else:
            algo, w = lims[lim]
            state = used and holds_state(algo, b, c, x)
            if used:
                cls |= slot_values(algo, w, tag, a, b, c, x) - {DEAD_MARK}
        rep["state_slots"] += state
        rep["tombstones"] += used and not state
        _count(rep, cls, i)
    return rep


def add_reports(p, q):
    """What the reports of two disjoint ranges must add up to."""
    out = {f: p[f] + q[f] for f in ("regions", "slots", "used_slots", "state_slots", "tombstones",
                                    "cache_words", "bad_slots")}
    out["violations"] = [x + y for x, y in zip(p["violations"], q["violations"])]
    out["first"] = [min(x, y) for x, y in zip(p["first"], q["first"])]
    return out


# ---------------------------------------------------------------------------- placement model
class Table:
    def __init__(self, bits=BITS, cache=False):
        self.bits = bits
        self.slots = np.zeros((1 << bits, NS, 4), np.uint64)
        self.cache = np.zeros((1 << bits, NS), np.uint64) if cache else None

    def used(self, r, s):
        return bool(self.slots[r, s].any() or (self.cache is not None and self.cache[r, s]))

    def set(self, r, s, tag, words, x=0):
        self.slots[r, s] = [tag] + list(words)
        if self.cache is not None:
            self.cache[r, s] = x
        else:
            assert x == 0

    def free(self, r, s):
        self.set(r, s, 0, (0, 0, 0))

    def put(self, tag, words, x=0):
        """As every writer places a key: the first free slot from its home in its region."""
        r = region_local(tag, 0, self.bits)
        s = slot_home(tag)
        for _ in range(NS):
            if not self.used(r, s):
                self.set(r, s, tag, words, x)
                return r, s
            s = (s + 1) % NS
        raise RuntimeError("region full")

    def copy(self):
        t = Table(self.bits, self.cache is not None)
        t.slots[:] = self.slots
        if self.cache is not None:
            t.cache[:] = self.cache
        return t


def make_tag(rng, region, home, bits=BITS):
    """A tag of `region` (its top bits) whose probe starts at `home` (4-aligned)."""
    low = 64 - bits
    mid = (int(rng.integers(1, 1 << 40)) << 12) & ((1 << low) - 1)
    return region << low | mid | (home & 252) | int(rng.integers(0, 4))


def f64_bits(v):
    return int(np.array([v], np.float64).view(np.uint64)[0])


def live_words(rng, algo):
    if algo == TB:
        return (f64_bits(float(rng.integers(0, MAXP)) + 0.25), T0 + int(rng.integers(0, 9000)), 1)
    c1, c0 = int(rng.integers(1, MAXP + 1)), int(rng.integers(0, MAXP + 1))
    o1, o0 = int(rng.integers(0, W)), int(rng.integers(0, W))
    return (T0 + W * int(rng.integers(0, 3)), c1 | c0 << 32, o1 | o0 << 32)


def dead_words(rng, algo):
    """A tombstone: a reset key (TB: zeros; SW: both counts zero, start and offsets stale)."""
    if algo == TB:
        return (0, 0, 0)
    return (T0 + W * int(rng.integers(0, 3)), 0, int(rng.integers(0, W)))


FILLS = (30, 0, 0, 130, 200, 255, 256, 5)    # keys per region: two empty ... one free slot, full


def healthy_table(seed, algo, cache=False, fills=FILLS, bits=BITS):
    """Keys placed by linear probing, a fifth of them tombstones, some blocked by a cache word;
    region 0 holds tag 0 (TB: dead, so it carries the mark)."""
    rng = np.random.default_rng(seed)
    t = Table(bits, cache)
    for r in range(1 << bits):
        n = fills[r % len(fills)]
        if r == 0 and n < NS:
            t.put(0, (0, 0, DEAD) if algo == TB else live_words(rng, algo))
        for i in range(n - t_used(t, r)):
            # clustered homes, so that chains collide and wrap past slot 255
            home = int(rng.choice([0, 4, 128, 248, 252])) if i % 2 else int(rng.integers(0, 64)) * 4
            dead = rng.random() < 0.2
            x = T0 + 5000 if cache and rng.random() < 0.1 else 0
            t.put(make_tag(rng, r, home, bits), dead_words(rng, algo) if dead else live_words(rng, algo), x)
    return t


def t_used(t, r):
    return sum(t.used(r, s) for s in range(NS))


# ---------------------------------------------------------------------------- corruptions
# Each returns (table, {class: (count, first)}): exactly these classes must be reported.
def corrupt_wrong_region(t, rng, r=3):
    s = next(s for s in range(NS) if t.used(r, s))
    tag = int(t.slots[r, s, 0])
    other = (r + 3) % (1 << t.bits)
    low = 64 - t.bits
    t.slots[r, s, 0] = other << low | (tag & ((1 << low) - 1))   # same home, same chain
    return t, {WRONG_REGION: (1, r << 8 | s)}


def corrupt_unreachable(t, rng, r=1, home=252):
    """Six keys of one home in an empty region (a chain that wraps for home 252), then a hole at
    the chain's fourth slot: the two keys behind it are lost."""
    assert t_used(t, r) == 0
    for _ in range(6):
        t.put(make_tag(rng, r, home, t.bits), (T0, 1, 0))
    t.free(r, (home + 3) % NS)
    lost = sorted(((home + 4) % NS, (home + 5) % NS))
    return t, {UNREACHABLE: (2, r << 8 | lost[0])}


def corrupt_duplicate(t, rng, algo=SW, r=2, home=8, wrap=False):
    """A key written twice: next to itself, or (wrap) at slot 254 and again at slot 0 behind a
    chain through slot 255, where the ORIGINAL has the higher index."""
    assert t_used(t, r) == 0
    words = (T0, 2, 7) if algo == SW else (f64_bits(2.0), T0, 1)
    if not wrap:
        tag = make_tag(rng, r, home, t.bits)
        t.set(r, home, tag, words)
        t.set(r, home + 1, tag, words)
        return t, {DUPLICATE: (1, r << 8 | (home + 1))}
    tags = [make_tag(rng, r, 252, t.bits) for _ in range(4)]
    for i, tag in enumerate(tags):
        t.set(r, 252 + i, tag, words)
    t.set(r, 0, tags[2], words)
    return t, {DUPLICATE: (1, r << 8 | 254)}


def corrupt_dead_mark(t, rng, r=3):
    s = next(s for s in range(NS) if t.used(r, s) and int(t.slots[r, s, 0]) != 0)
    t.slots[r, s, 3] = DEAD
    return t, {DEAD_MARK: (1, r << 8 | s)}


def _first_state(t, r, algo):
    return next(s for s in range(NS)
                if t.used(r, s) and holds_state(algo, int(t.slots[r, s, 2]), int(t.slots[r, s, 3]), 0)
                and int(t.slots[r, s, 2]) & 0xFFFFFFFF)


def corrupt_sw_start(t, rng, r=4):
    s = _first_state(t, r, SW)
    t.slots[r, s, 1] += np.uint64(1)
    return t, {SW_START: (1, r << 8 | s)}


def corrupt_sw_offset(t, rng, r=4):
    s = _first_state(t, r, SW)
    t.slots[r, s, 3] = (int(t.slots[r, s, 3]) & ~0xFFFFFFFF) | W      # newest bucket's offset = w
    return t, {SW_OFFSET: (1, r << 8 | s)}


def corrupt_tb_flags(t, rng, r=4):
    s = next(s for s in range(NS) if t.used(r, s) and int(t.slots[r, s, 3]) == 1)
    t.slots[r, s, 3] = 3
    return t, {TB_FLAGS: (1, r << 8 | s)}


def one_free_slot(rng, q, free_sub, bits=BITS, r=5):
    """Region r with every slot used by a key whose home is its own 4-slot bucket, except slot
    4q + free_sub. The slots of bucket q behind the free one are unreachable; nothing else is."""
    t = Table(bits)
    f = 4 * q + free_sub
    for s in range(NS):
        if s != f:
            t.set(r, s, make_tag(rng, r, s & 252, bits), (T0, 1, 0))
    lost = [s for s in range(f + 1, 4 * q + 4)]
    return t, ({UNREACHABLE: (len(lost), r << 8 | lost[0])} if lost else {})


def full_region(rng, bits=BITS, r=6):
    """No free slot: keys sit anywhere, far from their homes, and none is unreachable."""
    t = Table(bits)
    for s in range(NS):
        t.set(r, s, make_tag(rng, r, int(rng.integers(0, 64)) * 4, bits), (T0, 1, 0))
    return t, {}


def expect(t, algo, found):
    """The report a table must give whose only violations are `found` = {class: (count, first)}:
    the model's counters of what the table holds, and exactly those classes ("bad": the slots
    with a violation, where a slot counts in two classes)."""
    rep = check_model(t, algo)
    want = empty_report(rep["regions"], rep["slots"])
    for f in ("used_slots", "state_slots", "tombstones", "cache_words"):
        want[f] = rep[f]
    found = dict(found)
    bad = found.pop("bad", None)
    want["bad_slots"] = sum(n for n, _ in found.values()) if bad is None else bad
    for c, (n, first) in found.items():
        want["violations"][c] = n
        want["first"][c] = first
    return rep, want


def random_garbage(t, rng, n):
    """n slots overwritten with arbitrary words (and cache words): anything may be reported."""
    R = t.slots.shape[0]
    for _ in range(n):
        r, s = int(rng.integers(0, R)), int(rng.integers(0, NS))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            t.slots[r, s] = rng.integers(0, 1 << 63, 4, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        elif kind == 1:
            t.free(r, s)
        elif kind == 2:
            t.slots[r, s, 0] = t.slots[r, (s * 7) % NS, 0]              # some other slot's tag
        else:
            t.slots[r, s, 3] = int(rng.integers(0, 8))
        if t.cache is not None and rng.random() < 0.3:
            t.cache[r, s] = int(rng.integers(0, 3))
    return t


# ---------------------------------------------------------------------------- the case list
def structural_cases():
    """(name, algo, table, found): the shapes at which a checker can go wrong. found =
    {class: (count, first)} the table must report and nothing else; None: whatever the model says."""
    out = []
    rng = np.random.default_rng(2024)
    for algo, name in ((SW, "sw"), (TB, "tb")):
        for cache in (False, True) if algo == SW else (False,):
            tag = f"{name}{'+cache' if cache else ''}"
            base = healthy_table(7 + algo, algo, cache)
            out.append((f"healthy {tag}", algo, base, {}))
            out.append((f"wrong region {tag}", algo) + corrupt_wrong_region(base.copy(), rng))
            out.append((f"hole in a chain that wraps 255 -> 0 {tag}", algo) + corrupt_unreachable(base.copy(), rng))
            out.append((f"hole in a chain from home 8 {tag}", algo) + corrupt_unreachable(base.copy(), rng, home=8))
            out.append((f"duplicate next to itself {tag}", algo) + corrupt_duplicate(base.copy(), rng, algo))
            out.append((f"duplicate across the wrap {tag}", algo) + corrupt_duplicate(base.copy(), rng, algo, wrap=True))
        t, found = corrupt_dead_mark(healthy_table(11, algo), rng)
        out.append((f"dead mark on a keyed slot {name}", algo, t, found if algo == TB else {}))
    out.append(("sw start", SW) + corrupt_sw_start(healthy_table(12, SW), rng))
    out.append(("sw offset", SW) + corrupt_sw_offset(healthy_table(13, SW), rng))
    out.append(("tb flags", TB) + corrupt_tb_flags(healthy_table(14, TB), rng))
    out.append(("full region, keys far from home", SW) + full_region(rng))
    for q, sub, what in ((17, 1, "just before a key"), (17, 3, "just after a key"), (63, 0, "slot 252"),
                         (0, 0, "slot 0"), (63, 3, "slot 255")):
        out.append((f"one free slot, {what}", SW) + one_free_slot(rng, q, sub))
    # what a returning key leaves behind: its own expired slot further down the chain, behind the
    # slot it claimed. One ttl apart (to the millisecond) it is no duplicate; closer, it is one.
    for algo, ttl in ((SW, W), (TB, 2 * W)):
        for gap, dup in ((ttl + 1, False), (ttl, True), (0, True), (-ttl, True), (-ttl - 1, False)):
            t = Table()
            tag = make_tag(rng, 4, 16)
            for i, at in enumerate((T0 + 100 + gap, T0 + 100)):           # the new copy, then the stale one
                words = (T0, 3, at - T0) if algo == SW else (f64_bits(1.0), at, 1)
                if algo == SW and not 0 <= at - T0 < W:
                    words = (T0 + (at - T0) // W * W, 3, (at - T0) % W)
                t.set(4, 16 + i, tag, words)
            out.append((f"two copies {gap} ms apart {'sw' if algo == SW else 'tb'}", algo, t,
                        {DUPLICATE: (1, 4 << 8 | 17)} if dup else {}))
    t = Table()
    tag = make_tag(rng, 4, 16)
    t.set(4, 16, tag, (T0, 3, 5))
    t.set(4, 17, tag, (T0, 0, 5))                                         # a reset copy holds no state
    out.append(("a copy without state", SW, t, {}))
    # tag 0: with the mark (TB, dead), with state, the mark with a word beside it, and as the
    # all-zero slot that only its cache word keeps used
    t = Table()
    t.set(0, 0, 0, (0, 0, DEAD))
    out.append(("tag 0 dead with the mark", TB, t, {}))
    t = Table()
    t.set(0, 0, 0, (f64_bits(1.5), T0, 1))
    out.append(("tag 0 live", TB, t, {}))
    t = Table()
    t.set(0, 0, 0, (0, 9, DEAD))
    out.append(("tag 0, mark and a word", TB, t, {DEAD_MARK: (1, 0)}))
    t = Table(cache=True)
    t.set(0, 0, 0, (0, 0, 0), T0 + 9)
    out.append(("cache word only, at its home", SW, t, {}))
    t = Table(cache=True)
    t.set(0, 9, 0, (0, 0, 0), T0 + 9)
    out.append(("cache word only, behind free slots", SW, t, {UNREACHABLE: (1, 9)}))
    t = Table(cache=True)
    t.set(7, 255, 0, (0, 0, 0), T0 + 9)
    out.append(("cache word only, last slot of the table", SW, t, {UNREACHABLE: (1, 7 << 8 | 255),
                                                                  WRONG_REGION: (1, 7 << 8 | 255), "bad": 1}))
    # violations in the first and in the last region only
    t = healthy_table(15, SW, fills=(20, 40, 40, 40, 40, 40, 40, 20))
    for r in (0, 7):
        s = next(s for s in range(NS) if not t.used(r, s) and not t.used(r, (s - 1) % NS) and s % 4 == 3)
        t.set(r, s, make_tag(rng, r, s - 3), (T0, 1, 0))
    out.append(("first and last region only", SW, t, None))
    for seed in (1, 2):
        for algo in (SW, TB):
            t = random_garbage(healthy_table(20 + seed, algo, cache=algo == SW and seed == 1),
                               np.random.default_rng(seed), 60)
            out.append((f"random mix {seed} {'sw' if algo == SW else 'tb'}", algo, t, None))
    return out
