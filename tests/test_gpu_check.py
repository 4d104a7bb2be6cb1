"""rl_check_limiter(_device), rl_check_table_device, rl_check_images(_device): the device pass
that verifies a table's slot invariants, held to the Python restatement of the rules
(check_cases.check_model) on synthetic tables, and to the existing read paths (rl_limiter_usage,
rl_snapshot_keys, rl_copy_keys) on tables the engine's own writers produced.

Every engine has 8 regions per limiter to begin with (capacity 1) and may grow. Windows are 4000
ms, as in check_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import check_cases as cc
import rl_amd
from oracle.rl_oracle import PyOracle

pytestmark = pytest.mark.gpu

NS = 1_000_000
W, T0, MAXP = cc.W, cc.T0, cc.MAXP
IMG = rl_amd.KEY_IMAGE_DTYPE
CONFIGS = {"sw": dict(algo=rl_amd.SW, max_permits=MAXP, window_ms=W),
           "sw_cache": dict(algo=rl_amd.SW, max_permits=MAXP, window_ms=W, local_cache_ttl_ms=3000),
           "tb": dict(algo=rl_amd.TB, max_permits=MAXP, window_ms=W, refill_per_s=2.5)}
LIM = {"sw": 0, "sw_cache": 1, "tb": 2}
LIMS = [(cc.SW, W), (cc.SW, W), (cc.TB, W)]    # (algo, window_ms) of make()'s limiters


def make(names=("sw", "sw_cache", "tb"), **kw):
    kw.setdefault("max_batch", 1 << 16)
    e = rl_amd.Engine(capacity=1, **kw)
    for n in names:
        e.add_limiter(capacity=1, **CONFIGS[n])
    return e


@pytest.fixture(scope="module")
def eng():
    with make() as e:
        yield e


def new_report():
    out = torch.full((rl_amd.CHECK_WORDS,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()       # the fill runs on torch's stream, the check on the engine's
    return out


def fetch(e, out):
    e.sync()
    return rl_amd.check_dict(out.cpu().numpy())


def check_table(e, lim, t):
    slots = torch.from_numpy(t.slots.view(np.int64)).cuda()
    cache = torch.from_numpy(t.cache.view(np.int64)).cuda() if t.cache is not None else None
    torch.cuda.synchronize()
    out = new_report()
    e.check_table_device(lim, slots, cache, t.bits, out)
    return fetch(e, out)


# ---------------------------------------------------------------------------- 1. raw tables
CASES = cc.structural_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_raw_tables_against_the_model(eng, case):
    _, algo, t, found = case
    lim = LIM["tb"] if algo == cc.TB else LIM["sw_cache"] if t.cache is not None else LIM["sw"]
    want = cc.check_model(t, algo)
    if found is not None:
        assert want == cc.expect(t, algo, found)[1]
    assert check_table(eng, lim, t) == want


def test_a_table_of_64_regions_with_a_random_mix(eng):
    """More waves than one workgroup holds, violations in most regions: counts and first
    positions do not depend on which wave met them."""
    t = cc.random_garbage(cc.healthy_table(31, cc.SW, True, fills=(5, 60, 130, 200, 255, 256, 30, 0), bits=6),
                          np.random.default_rng(31), 300)
    want = cc.check_model(t, cc.SW)
    assert want["bad_slots"] > 100 and want["regions"] == 64
    assert check_table(eng, LIM["sw_cache"], t) == want
    # the same slots under the token bucket's rules, without the cache words
    t.cache = None
    assert check_table(eng, LIM["tb"], t) == cc.check_model(t, cc.TB)


# ---------------------------------------------------------------------------- 2. healthy engine paths
def region_of(key_hash, bits=3):
    return (rl_amd.mix64(key_hash) >> np.uint64(64 - bits)).astype(np.int64)


CAND = np.arange(1, 400_000, dtype=np.uint64)
REG = region_of(CAND)
KEYS = {r: CAND[REG == r] for r in range(8)}
GROUND = np.concatenate([KEYS[0][:110], KEYS[1][:110], KEYS[7][:5], np.array([0, 0xFFFFFFFFFFFFFFFF], np.uint64)])
BELOW, ABOVE = KEYS[2][:190], KEYS[3][:194]      # live + dead slots of a region: <= / > kTombCrowd = 192


def traffic(seed, keys, n, t_lo, t_hi, resets=0.03, regress=0.1):
    """n acquires (a few resets) over `keys` at times rising from t_lo to t_hi, a tenth of them
    sent back by up to a window (never before t_lo - 1000: the engines declare max_skew_ms 2000)."""
    rng = np.random.default_rng(seed)
    k = keys[rng.integers(0, keys.size, n)]
    now = np.sort(rng.integers(t_lo, t_hi, n))
    back = rng.random(n) < regress
    now[back] = np.maximum(now[back] - rng.integers(1, W, int(back.sum())), t_lo - 1000)
    ops = np.where(rng.random(n) < resets, rl_amd.OP_RESET, rl_amd.OP_ACQUIRE).astype(np.uint8)
    return k, rng.integers(1, 3, n).astype(np.int32), (now * NS).astype(np.int64), np.zeros(n, np.uint16), ops


def each_twice(keys, t):
    """Two acquires of every key at t and t + 1: > 96 records per region, so a batch loads the
    region as an image."""
    k = np.concatenate([keys, keys])
    now = np.concatenate([np.full(keys.size, t), np.full(keys.size, t + 1)]) * NS
    return k, np.ones(k.size, np.int32), now.astype(np.int64), np.zeros(k.size, np.uint16), np.zeros(k.size, np.uint8)


class Healthy:
    """An engine with one limiter and the oracle fed the same batches; sound() holds the checker
    to the three existing read paths."""

    def __init__(self, name):
        self.name = name
        self.e = make((name,), max_skew_ms=2000)
        self.o = PyOracle()
        self.o.add_limiter(**CONFIGS[name])
        self.now = T0
        self.seen = set()

    def run(self, tr):
        st = self.e.execute(*tr)[3]
        assert st == rl_amd.RL_OK, rl_amd.strerror(st)
        self.o.run(*tr)
        self.now = max(self.now, int(tr[2].max()) // NS)
        self.seen |= set(int(k) for k in tr[0])

    def sound(self, what, e=None, gone=()):
        e = e or self.e
        rep = e.check_limiter(0)
        assert rep["bad_slots"] == 0 and not any(rep["violations"]), (what, rep)
        assert rep["first"] == [rl_amd.CHECK_NONE] * rl_amd.CHECK_CLASSES, what
        assert rep["slots"] == e.limiter_slots(0) == rep["regions"] * 256, what
        assert rep["used_slots"] == e.limiter_usage(0, self.now * NS)["used_slots"], what
        assert rep["state_slots"] == sum(len(c) for c in e.snapshot(0, chunk=1 << 12)), what
        assert rep["tombstones"] == rep["used_slots"] - rep["state_slots"], what
        live = {k for _, k, *_ in self.o.keyspace(self.now)} - set(gone)
        held = set(int(k) for k in e.copy_keys(np.array(sorted(self.seen), np.uint64))["key_hash"])
        assert live <= held, (what, sorted(live - held)[:5])
        return rep


@pytest.mark.parametrize("name", ["sw", "sw_cache", "tb"])
def test_healthy_engine_paths_report_nothing(name):
    h = Healthy(name)
    e = h.e
    h.run(traffic(1, GROUND, 3000, T0 + 500, T0 + 3 * W))            # rollovers, resets, regression
    assert h.sound("batches")["used_slots"] > 200
    h.run(traffic(2, GROUND, 3000, T0 + 3 * W, T0 + 5 * W))
    h.sound("more batches")
    t1 = T0 + 20 * W                                                 # everything above is dead by now
    h.run(traffic(3, GROUND[::7], 400, t1, t1 + W, resets=0))
    h.sound("ttl expiry")
    # one region just below, one just above kTombCrowd live + dead slots, then the keys come back
    h.run(each_twice(np.concatenate([BELOW, ABOVE]), t1 + W))
    h.sound("crowded regions filled")
    t2 = t1 + 20 * W
    h.run(each_twice(np.concatenate([BELOW[::3], ABOVE[::3], KEYS[2][190:230], KEYS[3][194:200]]), t2))
    h.sound("crowded regions reloaded")
    # region 2 (190 dead slots at the load) kept them in place; region 3 (194) dropped them and relinked
    assert e.check_limiter(0, 2, 1)["used_slots"] >= 190
    assert e.check_limiter(0, 3, 1)["used_slots"] < 150
    h.run(each_twice(np.concatenate([BELOW[1::3], ABOVE[1::3]]), t2 + 10 * W))
    h.sound("crowded regions reloaded again")
    h.run(traffic(4, np.concatenate([GROUND, BELOW, ABOVE]), 3000, t2 + 11 * W, t2 + 13 * W))
    h.sound("mixed traffic over tombstones")
    slots = e.limiter_slots(0)
    e.grow_limiter(0, slots)                                         # load <= 0.5: twice the slots
    assert e.limiter_slots(0) == 2 * slots
    h.sound("grow")
    h.run(traffic(5, np.concatenate([GROUND, BELOW]), 2000, t2 + 13 * W, t2 + 14 * W))
    h.sound("batch after grow")
    e.sweep_expired(h.now * NS)
    assert h.sound("sweep")["tombstones"] == 0                       # what a sweep keeps holds state
    h.run(traffic(6, GROUND, 2000, t2 + 14 * W, t2 + 15 * W))
    e.shrink_limiter(0, h.now * NS)
    h.sound("shrink")
    entries = e.export_state(h.now * NS)
    assert len(entries) > 50
    st, taken = e.import_state(entries)
    assert st == rl_amd.RL_OK and taken == len(entries)
    h.sound("import of its own export")
    some = np.array(sorted(h.seen), np.uint64)[::5]
    imgs = e.copy_keys(some)
    assert len(imgs) > 10 and e.drop_keys(some) == len(imgs)
    h.sound("drop", gone=set(int(k) for k in some))
    assert e.put_keys(imgs) == (rl_amd.RL_OK, len(imgs))
    h.sound("put")
    # snapshot -> ordered put into a second engine with the same table size. (Since the sweep no
    # batch has started later than the state it found was live, so no key has come back after its
    # TTL and left an expired slot behind the one it claimed: a snapshot of such a table holds two
    # images of the key, which is the restore path's business and not the checker's)
    with make((name,), max_skew_ms=2000) as b:
        b.grow_limiter(0, e.limiter_slots(0) // 2)
        assert b.limiter_slots(0) == e.limiter_slots(0)
        snap = np.concatenate(list(e.snapshot(0)))
        dev = torch.from_numpy(snap.view(np.uint8).copy()).cuda()
        hdr = torch.zeros(4, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        b.put_keys_device(len(snap), dev, hdr)
        b.sync()
        assert hdr.cpu().tolist() == [len(snap), 0, 0, len(snap)]
        rep = h.sound("restored engine", e=b)
        assert rep["state_slots"] == len(snap) and rep["tombstones"] == 0
    e.close()


def test_states_only_an_import_can_produce_pass():
    """rl_import_state admits bucket counts above max_permits and any double as a balance; the
    checker must not call such a table corrupt (the reserved classes SW_COUNT and TB_TOKENS)."""
    with make() as e:
        ent = np.zeros(6, rl_amd.STATE_DTYPE)
        ent["key_hash"] = [11, 11, 12, 21, 22, 23]
        ent["limiter"] = [0, 0, 1, 2, 2, 2]
        ent["kind"] = [0, 0, 0, 1, 1, 1]
        ent["window_start_ms"][:3] = [T0 + W, T0, T0]
        ent["count"][:3] = [MAXP + 50, 0xFFFFFFFF, 1]
        ent["expire_at_ms"][:3] = [T0 + 2 * W + 7, T0 + W, T0 + 2 * W - 1]      # offsets 7, 0, w - 1
        ent["tokens"][3:] = [float("nan"), -5.5, 1e300]
        ent["last_refill_ms"][3:] = T0
        ent["expire_at_ms"][3:] = T0 + 2 * W
        assert e.import_state(ent) == (rl_amd.RL_OK, 6)
        for lim, n in ((0, 1), (1, 1), (2, 3)):
            rep = e.check_limiter(lim)
            assert rep["bad_slots"] == 0 and rep["state_slots"] == n == rep["used_slots"]


def test_negative_clock_is_not_a_violation():
    """now < 0: Java's truncating division gives window starts that are multiples of w and
    offsets in (-w, 0]."""
    with make(("sw",)) as e:
        now = (np.array([-3 * W - 1, -3 * W - 1, -2 * W - 3999, -5, -1]) * NS).astype(np.int64)
        keys = np.array([5, 6, 5, 7, 7], np.uint64)
        st = e.execute(keys, np.ones(5, np.int32), now)[3]
        assert st == rl_amd.RL_OK
        rep = e.check_limiter(0)
        assert rep["bad_slots"] == 0 and rep["state_slots"] == 3


# ---------------------------------------------------------------------------- 3. value classes on a real table
def image(key, words, x=0, lim=0, reserved=0):
    im = np.zeros(1, IMG)
    im["key_hash"], im["word"], im["cache_word"], im["limiter"] = key, [w & cc.M64 for w in words], x, lim
    im["reserved"][0, 2] = reserved
    return im


def distinct_homes(n, start=1):
    """Keys whose (region, home) pairs are all different, so each sits at its home in an empty
    table: position = region << 8 | home."""
    out, seen = [], set()
    for k in range(start, start + 100_000):
        tag = cc.mix64(k)
        at = (cc.region_local(tag, 0, 3), cc.slot_home(tag))
        if at not in seen:
            seen.add(at)
            out.append((k, at[0] << 8 | at[1]))
            if len(out) == n:
                return out
    raise AssertionError


def crafted():
    """(images, {limiter: {class: [key positions]}}): every checked value class on limiters 0
    (sliding window) and 2 (token bucket), among good images."""
    ks = distinct_homes(24)
    sw = lambda c1, c0, o1, o0: (c1 | c0 << 32, (o1 & 0xFFFFFFFF) | (o0 & 0xFFFFFFFF) << 32)  # noqa: E731
    rows = [  # (limiter, words, cache word, classes)
        (0, (T0,) + sw(3, 2, 10, 3999), 0, ()),
        (0, (T0 + 1,) + sw(3, 0, 10, 0), 0, (cc.SW_START,)),
        (0, (T0 - 1,) + sw(0, 1, 0, 5), 0, (cc.SW_START,)),
        (0, (T0 + 1,) + sw(0, 0, 9, 9), 0, ()),                       # a tombstone: nothing to check
        (0, (T0,) + sw(1, 0, W, 0), 0, (cc.SW_OFFSET,)),
        (0, (T0,) + sw(1, 1, 0, -W), 0, (cc.SW_OFFSET,)),
        (0, (T0,) + sw(0, 1, W, W + 1), 0, (cc.SW_OFFSET,)),
        (0, (T0,) + sw(1, 0, W - 1, W), 0, ()),                       # the empty bucket's offset is stale
        (0, (T0 + 2,) + sw(2, 2, -W, 1), 0, (cc.SW_START, cc.SW_OFFSET)),
        (0, (T0,) + sw(MAXP + 9, 0, cc.DEAD, 0), 0, ()),              # c == 2 and a count above max: fine
        (2, (cc.f64_bits(2.5), T0, 1), 0, ()),
        (2, (cc.f64_bits(-1.0), T0, 1), 0, ()),
        (2, (cc.f64_bits(2.5), T0, 3), 0, (cc.TB_FLAGS,)),
        (2, (cc.f64_bits(2.5), T0, 4), 0, (cc.TB_FLAGS,)),
        (2, (0, 0, 1 << 63), 0, (cc.TB_FLAGS,)),
        (2, (0, 0, cc.DEAD), 0, (cc.DEAD_MARK,)),                     # the mark on a key that is not 0
        (2, (0, T0, cc.DEAD), 0, (cc.DEAD_MARK,)),
        (2, (0, 0, 0), 0, None),                                      # all zero but the tag: a tombstone
    ]
    imgs, want = [], {0: {}, 2: {}}
    for (k, pos), (lim, words, x, classes) in zip(ks, rows):
        imgs.append(image(k, words, x, lim))
        for c in classes or ():
            want[lim].setdefault(c, []).append(pos)
    imgs.append(image(0, (0, 0, cc.DEAD), 0, 2))                      # key 0, dead: the mark where it belongs
    return np.concatenate(imgs), want


def test_value_classes_on_a_real_table():
    imgs, want = crafted()
    with make() as e:                                                 # no batch ever runs on it
        assert e.put_keys(imgs) == (rl_amd.RL_OK, len(imgs))
        for lim in (0, 1, 2):
            rep = e.check_limiter(lim)
            n = int((imgs["limiter"] == lim).sum())
            assert rep["used_slots"] == n and (rep["regions"], rep["slots"]) == (8, 2048)
            exp = want.get(lim, {})
            bad = set(p for ps in exp.values() for p in ps)
            assert rep["bad_slots"] == len(bad)
            for c in range(rl_amd.CHECK_CLASSES):
                ps = exp.get(c, [])
                assert rep["violations"][c] == len(ps), (lim, c)
                assert rep["first"][c] == (min(ps) if ps else rl_amd.CHECK_NONE), (lim, c)
            algo = LIMS[lim][0]
            mine = imgs[imgs["limiter"] == lim]
            assert rep["state_slots"] == sum(cc.holds_state(algo, int(i["word"][1]), int(i["word"][2]), 0) for i in mine)
            assert rep["tombstones"] == n - rep["state_slots"]


# ---------------------------------------------------------------------------- 4. image lists


def check_images_both(e, imgs):
    host = e.check_images(imgs)
    dev = torch.from_numpy(np.ascontiguousarray(imgs).view(np.uint8).copy()).cuda() if len(imgs) else None
    torch.cuda.synchronize()
    out = new_report()
    e.check_images_device(len(imgs), dev, out)
    assert fetch(e, out) == host
    return host


def test_check_images():
    imgs, _ = crafted()
    extra = np.concatenate([image(77, (T0, 1, 0), lim=3), image(78, (T0 + 1, 1, 0), lim=9),     # no such limiter
                            image(79, (T0, 1, 0), lim=0, reserved=1),
                            image(80, (T0 + 1, 1, W), lim=1, reserved=7),                       # three classes at once
                            image(81, (0, 0, 0), x=T0 + 5, lim=1), image(0, (0, 0, 0), lim=0)])  # cache word only; all zero
    lst = np.concatenate([imgs, extra])
    with make() as e:
        assert check_images_both(e, np.zeros(0, IMG)) == cc.empty_report(0, 0)
        rep = check_images_both(e, lst)
        assert rep == cc.check_images_model(lst, LIMS)
        assert rep["violations"][cc.IMAGE_LIMITER] == 2 and rep["first"][cc.IMAGE_LIMITER] == len(imgs)
        assert rep["violations"][cc.IMAGE_RESERVED] == 2 and rep["violations"][cc.DEAD_MARK] == 0
        assert rep["violations"][cc.SW_START] == 4 and rep["slots"] == len(lst) == rep["used_slots"] + 1
        # the snapshot of a healthy engine passes, and every image of it holds state
        e.execute(*traffic(9, GROUND, 2000, T0, T0 + 2 * W)[:3])
        snap = np.concatenate(list(e.snapshot(0)))
        rep = check_images_both(e, snap)
        assert rep["bad_slots"] == 0 and rep["state_slots"] == rep["used_slots"] == len(snap) > 100


def test_check_images_stages_a_list_longer_than_max_batch():
    rng = np.random.default_rng(4)
    n = 2500
    lst = np.zeros(n, IMG)
    lst["key_hash"] = rng.integers(1, 1 << 60, n)
    lst["limiter"] = rng.integers(0, 3, n)
    sw = lst["limiter"] < 2
    lst["word"][sw, 0] = T0
    lst["word"][sw, 1] = 1
    lst["word"][~sw, 2] = 1
    lst["word"][2100, 0] += 1 if sw[2100] else 0                       # the only bad start, in the third piece
    lst["limiter"][[1030, 2499]] = 5
    lst["reserved"][[7, 1023, 1024], 1] = 1
    with make(max_batch=1024) as e:
        rep = check_images_both(e, lst)
    assert rep == cc.check_images_model(lst, LIMS)
    assert rep["first"][cc.IMAGE_LIMITER] == 1030 and rep["violations"][cc.IMAGE_LIMITER] == 2
    assert rep["first"][cc.IMAGE_RESERVED] == 7 and rep["violations"][cc.IMAGE_RESERVED] == 3
    if sw[2100]:
        assert rep["first"][cc.SW_START] == 2100


# ---------------------------------------------------------------------------- 5. ranges, streams, read-only
def test_ranges_add_up_streams_agree_and_nothing_else_changes():
    imgs, _ = crafted()
    with make() as e:
        e.execute(*traffic(8, np.concatenate([GROUND, BELOW]), 3000, T0, T0 + 2 * W)[:3])
        assert e.put_keys(imgs[imgs["limiter"] == 0])[0] == rl_amd.RL_OK        # some violations to find
        before = (e.stats(), e.last_status(), e.limiter_usage(0, (T0 + 2 * W) * NS), np.concatenate(list(e.snapshot(0))))
        whole = e.check_limiter(0)
        assert whole["bad_slots"] == 6 and whole["regions"] == 8
        for cut in (0, 1, 4, 7, 8):
            lo, hi = e.check_limiter(0, 0, cut), e.check_limiter(0, cut)
            assert (lo["regions"], hi["regions"]) == (cut, 8 - cut)
            assert cc.add_reports(lo, hi) == whole
        assert e.check_limiter(0, 3, 2) == cc.add_reports(e.check_limiter(0, 3, 1), e.check_limiter(0, 4, 1))
        for begin in (8, 9, 1 << 40):
            assert e.check_limiter(0, begin, 5) == cc.empty_report(0, 0)
        # the device form, on the engine's stream and on a caller's
        out = new_report()
        e.check_limiter_device(0, 0, 1 << 62, out)
        assert fetch(e, out) == whole
        s = torch.cuda.Stream()
        out2, out3 = new_report(), new_report()
        torch.cuda.synchronize()
        e.check_limiter_device(0, 2, 3, out2, stream=s.cuda_stream)
        e.check_limiter_device(0, 99, 3, out3, stream=s.cuda_stream)
        s.synchronize()
        assert rl_amd.check_dict(out2.cpu().numpy()) == e.check_limiter(0, 2, 3)
        assert rl_amd.check_dict(out3.cpu().numpy()) == cc.empty_report(0, 0)
        e.check_images(imgs)
        after = (e.stats(), e.last_status(), e.limiter_usage(0, (T0 + 2 * W) * NS), np.concatenate(list(e.snapshot(0))))
        assert before[:3] == after[:3] and np.array_equal(before[3], after[3])


def test_argument_errors_with_an_engine():
    with make() as e:
        L, h = rl_amd.lib(), e.handle
        r = rl_amd.CheckReport()
        ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
        before = bytes(r)
        assert L.rl_check_limiter(h, 3, 0, 8, ctypes.byref(r)) == rl_amd.RL_E_INVALID_ARG     # an unknown limiter
        assert L.rl_check_images(h, (1 << 31) + 1, ctypes.byref(r), ctypes.byref(r)) == rl_amd.RL_E_TOO_LARGE
        assert bytes(r) == before
        out = new_report()
        with pytest.raises(rl_amd.RlError):
            e.check_limiter_device(3, 0, 8, out)
        with pytest.raises(rl_amd.RlError):
            e.check_table_device(0, out, None, 2, out)
        e.sync()
        assert out.cpu().tolist() == [0x5A5A5A5A] * rl_amd.CHECK_WORDS
