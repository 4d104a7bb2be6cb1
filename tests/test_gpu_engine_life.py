"""One engine over a changing life, bit-exact against the oracle batch by batch (the cases:
tests/life_cases.py; that they are meaningful: tests/test_life_cases_model.py).

Every case is one engine and one continuing trace. Between its batches the sizes fall and rise, the
records turn wide and compact again, the hot path, routing, walks, segments and the region order
are switched off and on, the table crosses from one partition pass to two and back, the hot marks'
epoch wraps, and queries run on scratch that an earlier, larger call sized: each of these leaves
stale words in a reused buffer, and a kernel that read one would decide differently
from the oracle here. Every case also asserts, from the engine's own counters, that the path it is
named after ran."""
import numpy as np
import pytest

import life_cases as lc
import rl_amd
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


def total_regions(e, n_lim):
    return sum(e.limiter_slots(l) for l in range(n_lim)) // rl_amd.REGION_SLOTS


def to_device(tr):
    import torch
    k, p, t, l, o = tr
    return [torch.from_numpy(np.array(x)).cuda()      # (a copy: the cases' arrays are read-only)
            for x in (k.view(np.int64), p, t, l.view(np.int16), o)]


def enqueue_device(e, b):
    """The batch through rl_execute_batch_device on caller tensors of exactly n elements."""
    import torch
    n = len(b.tr[0])
    dev = to_device(b.tr)
    a = torch.empty(n, dtype=torch.uint8, device="cuda")
    r = torch.empty(n, dtype=torch.int64, device="cuda")
    t = torch.empty(n, dtype=torch.float64, device="cuda") if b.want_tokens else None
    torch.cuda.synchronize()                      # the inputs are complete (no stream is passed)
    e.execute_device(n, *dev, a, r, t)
    return dev, a, r, t


def check_status(st, w, what):
    assert st == (rl_amd.RL_E_INVALID_REQUEST if w[3] else rl_amd.RL_OK), f"{what}: {rl_amd.strerror(st)}"


def check_counters(e, b, w, hits_before, what):
    s = e.stats()
    if b.hot is not None:
        assert (s["hot_regions"] >= 1) == b.hot, f"{what}: hot_regions {s['hot_regions']}"
    if b.routed is not None:
        assert (s["routed"] > 0) == b.routed, f"{what}: routed {s['routed']}"
    if b.cache_hits:
        assert s["cache_hits"] == w[4] - hits_before > 0, f"{what}: cache_hits {s['cache_hits']}"


def run_case(name, between=None, stats_out=None):
    """Runs the case on a fresh engine; returns every batch's (allowed, remaining, tokens).
    between(engine, batch_index): called after every checked batch (the queries of case 9).
    stats_out: a list that receives every batch's statistics instead of the counters' assertions
    (measurement)."""
    case, want = lc.get(name)
    per = case.capacity // len(case.limiters)
    e = rl_amd.Engine(max_batch=case.max_batch, capacity=case.capacity, pipeline=case.pipeline)
    out, pending = [], []
    try:
        def add(l):
            e.add_limiter(*l[:4], capacity=per, local_cache_ttl_ms=l[5] if len(l) > 5 else 0)

        for l in case.limiters:
            add(l)
        n_lim = len(case.limiters)
        if case.tile_items:
            e.tune("tile_items", case.tile_items)
        for k, v in case.tune.items():
            e.tune(k, v)
        i, last_now = 0, lc.T0 * lc.NS
        for s in case.steps:
            if s[0] == "tune":
                e.tune(s[1], s[2])
            elif s[0] == "grow":
                before = e.limiter_slots(s[1])
                e.grow_limiter(s[1], s[2])
                assert e.limiter_slots(s[1]) > before and e.stats()["table_grows"] >= 1
            elif s[0] == "shrink":
                before = e.limiter_slots(s[1])
                rep = e.shrink_limiter(s[1], last_now, s[2])
                assert rep["halvings"] > 0 and e.limiter_slots(s[1]) == rep["slots_after"] < before, rep
            elif s[0] == "add_limiter":
                add(s[1])
                n_lim += 1
            elif s[0] == "width":
                assert e.result_width() == s[1], (name, s)
            elif s[0] == "regions":
                assert (total_regions(e, n_lim) > lc.MAX_ONE_PASS_REGIONS) == (s[1] == "two"), (name, s)
            elif s[0] == "batch":
                b, w = s[1], want[i]
                what = f"{name} batch {i} {b.note}"
                last_now = int(b.tr[2].max()) if int(b.tr[2].max()) < (lc.T0 + (1 << 32)) * lc.NS else last_now
                if case.pipeline:
                    pending.append((i, b, enqueue_device(e, b)))     # no sync between the calls
                else:
                    if b.entry == "device":
                        _, a, r, t = enqueue_device(e, b)
                        check_status(e.last_status(), w, what)
                        got = (a.cpu().numpy(), r.cpu().numpy(), None if t is None else t.cpu().numpy())
                    else:
                        a, r, t, st = e.execute(*b.tr, want_tokens=b.want_tokens)
                        check_status(st, w, what)
                        got = (a, r, t)
                    assert_same(got, w, what)
                    if stats_out is not None:
                        stats_out.append(e.stats())
                    else:
                        check_counters(e, b, w, want[i - 1][4] if i else 0, what)
                    out.append(got)
                    if between:
                        between(e, i)
                i += 1
        if pending:
            e.sync()
            check_status(e.last_status(), want[pending[-1][0]], f"{name}: the last batch")
            for i, b, (_, a, r, t) in pending:
                got = (a.cpu().numpy(), r.cpu().numpy(), None if t is None else t.cpu().numpy())
                assert_same(got, want[i], f"{name} batch {i} (pipelined)")
                out.append(got)
            i, b, _ = pending[-1]
            check_counters(e, b, want[i], want[i - 1][4] if i else 0, f"{name}: the last batch")
    finally:
        e.close()
    return out


@pytest.mark.parametrize("name", [n for n in lc.CASES])
def test_life(name):
    run_case(name)


# ---------------------------------------------------------------- 9. queries on shared scratch
QUERY_AFTER = (0, 3, 4, 7)                        # after the batches of 66,049, 63, 12,801 and 66,049


def run_queries_case():
    """Case 1 with the queries between its batches, each made twice, the second time with the
    smaller argument (their scratch is shared and sized by the largest call so far). Each answer is
    checked against the host model its own test file uses; the Python oracle runs in step for the
    table's content. The queries only read: the batches after them stay bit-exact."""
    import check_cases as cc
    import report_cases as rc
    import test_gpu_digest as tdig
    import test_gpu_keys as tkeys
    import test_gpu_retry_after as tra
    import test_gpu_top_keys as ttop
    import test_gpu_usage as tu
    from oracle.rl_oracle import PyOracle

    case, want = lc.get("sizes-split1")
    batches = case.batches()
    lims6 = [tuple(l) + (0, 0) for l in case.limiters]
    po = PyOracle()
    for l in lims6:
        po.add_limiter(*l)
    n_lim = len(lims6)
    rng = np.random.default_rng(9)
    words = [f"tenant-{i}:user-{int(x)}".encode() for i, x in enumerate(rng.integers(0, 10**9, 1500))]
    blob, off = rl_amd.pack_keys(words)
    want_hash = tkeys.host_hashes(np.asarray(blob), np.asarray(off))[0]
    done = []

    def between(e, i):
        b, w = batches[i], want[i]
        keys, permits, now, lim, op = b.tr
        po.run(*b.tr)                               # the Python twin, for the models that read its keyspace
        if i not in QUERY_AFTER:
            return
        now_ms = int(now.max()) // lc.NS + 1
        big, small = QUERY_AFTER[0], i
        bk = batches[big].tr[0]
        # top_keys: n large, then small (device and host forms)
        ttop.check(e, bk, 4096, 1)
        ttop.check(e, keys[:max(len(keys) // 16, 1)], 7, 1)
        # tally_batch / top_denied on the finished batch, then on its first part
        for m in (len(keys), max(len(keys) // 8, 1)):
            args = (permits[:m], lim[:m], op[:m], w[0][:m], w[1][:m])
            got = e.tally_batch(*args)
            assert got.tobytes() == rc.tally_model(n_lim, *args).tobytes(), (i, m)
            for sel in range(n_lim):
                gk, gc, gh, gd = e.top_denied(keys[:m], *args, sel, 64, 1)
                wk, wc, wh, wd = rc.top_denied_model(n_lim, keys[:m], *args, sel, 64, 1)
                assert (gh, gd) == (wh, wd) and np.array_equal(gk, wk) and np.array_equal(gc, wc), (i, m, sel)
        for lid in range(n_lim):
            mx = lims6[lid][1]
            # limiter_usage / top_consumers: k large, then small
            census, order = tu.expected(po, lid, now_ms, lims6)
            got = tu.check_census(e, lid, now_ms, census)
            tu.check_top(e, lid, now_ms, order, mx, ks=(4096, 7))
            # limiter_digest: as many buckets as regions, then two (the "largest so far" buffer)
            ent = [x for x in po.keyspace(now_ms) if x[0] == lid]
            for bits in (tdig.region_bits(e, lid), 1):
                d, tot = e.limiter_digest(lid, now_ms * lc.NS, bits, cache=False)
                model = rl_amd.digest_model(ent, [], 1, bits)
                assert tdig.raw(d) == tdig.raw(model) and tot == tdig.total_of(model), (i, lid, bits)
            # snapshot_keys: the whole table, then a cap of two regions (whole regions, the same prefix)
            full, st, n_full, reg, total = e.snapshot_keys(lid, 0, 1 << 62, 1 << 15)
            assert st == rl_amd.RL_OK and reg == total == e.limiter_slots(lid) // rl_amd.REGION_SLOTS
            assert n_full >= census["live_keys"] and (full["limiter"][:n_full] == lid).all()
            part, st, n_part, reg2, _ = e.snapshot_keys(lid, 0, 1 << 62, 2 * rl_amd.REGION_SLOTS)
            assert st == rl_amd.RL_OK and 0 < reg2 < total and n_part <= 2 * rl_amd.REGION_SLOTS
            assert part[:n_part].tobytes() == full[:n_part].tobytes() and not part[n_part:]["key_hash"].any()
            assert {int(x[1]) for x in ent} <= set(full["key_hash"][:n_full].tolist())   # every live key
            # check_images on what the snapshot gave (the staging of a larger call, then a smaller)
            cl = [(l[0], l[2]) for l in lims6]
            for imgs in (full[:n_full], full[:max(n_full // 9, 1)]):
                assert e.check_images(imgs) == cc.check_images_model(imgs, cl), (i, lid, len(imgs))
            # check_limiter: the whole table, then three regions
            rep = e.check_limiter(lid)
            assert rep["bad_slots"] == 0 and not any(rep["violations"]), rep
            assert rep["regions"] == total and rep["slots"] == e.limiter_slots(lid)
            assert rep["used_slots"] == got["used_slots"]
            rep3 = e.check_limiter(lid, 1, 3)
            assert rep3["bad_slots"] == 0 and rep3["regions"] == 3 and rep3["used_slots"] <= rep["used_slots"]
            rest = cc.add_reports(e.check_limiter(lid, 0, 1), e.check_limiter(lid, 4))
            assert cc.add_reports(rep3, rest) == rep, (i, lid)   # disjoint ranges add up (check_cases)
            # retry_after: the busiest keys of the limiter, then one of them
            mine = keys[(lim == lid) & (op == 0) & (permits > 0)]
            u, c = np.unique(mine, return_counts=True)
            qk = u[np.argsort(-c, kind="stable")][:3] if i != 3 else u[:1]
            for kk in (qk, qk[:1]):
                wait, st = e.retry_after(lid, kk, 2, now_ms * lc.NS)
                assert st == rl_amd.RL_OK
                for key, wt in zip(kk.tolist(), wait.tolist()):
                    assert [wt] == tra.scan_waits(po, lid, key, [2], now_ms), (i, lid, key)
        # hash_keys / execute_batch_keys (peeks: read-only): a 16 KiB blob stage, then 4 KiB
        peek = np.full(len(words), rl_amd.OP_PEEK, np.uint8)
        ones, at = np.ones(len(words), np.int32), np.full(len(words), now_ms * lc.NS, np.int64)
        wl = (np.arange(len(words)) % n_lim).astype(np.uint16)
        for stage in (16384, 4096):
            e.tune("key_stage_bytes", stage)
            assert np.array_equal(e.hash_keys(blob, off), want_hash), (i, stage)
            a, r, _, st, h = e.execute_batch_keys(blob, off, ones, at, wl, peek, want_tokens=False)
            wa, wr, _ = po.run(want_hash, ones, at, wl, peek)
            assert st == rl_amd.RL_OK and np.array_equal(h, want_hash)
            assert np.array_equal(r, np.asarray(wr, np.int64)), (i, stage)
            assert np.array_equal(a, np.asarray(wa, np.uint8)), (i, stage)
        done.append(i)

    run_case("sizes-split1", between=between)
    assert tuple(done) == QUERY_AFTER


def test_queries_on_shared_scratch():
    run_queries_case()
