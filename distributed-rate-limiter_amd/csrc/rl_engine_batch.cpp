// rl_engine_batch.cpp — a batch: its scratch, the launch chain (run_batch_device), the status
// it leaves behind, and the calls that run one (rl_execute_batch(_device), peek and reset).
// The arithmetic of a batch is rl_batch_plan.hpp. A batch of at most rl_tune("small_batch")
// requests takes one launch instead of the chain (small_route, run_small, run_small_host; the
// kernel: rl_small.hip).
#include "rl_engine_impl.hpp"
#include "rl_small.hpp"

using namespace rl;

static bool scratch_fits(const BatchScratch& B, size_t n, bool wide) {
    return n <= B.cap_n && (!wide || B.cap_wide);
}

// The per-request arrays of a set, and its [bin][tile] counts.
static int ensure_scratch(rl_engine* e, BatchScratch& B, size_t n, bool wide, size_t counts_words) {
    if (!scratch_fits(B, n, wide)) {
        // sized for this batch (+1/8 headroom), not max_batch: a router's engine accepts up
        // to its receive capacity but usually sees about its per-rank share
        size_t cap = std::max<size_t>(n, std::min<size_t>(e->opts.max_batch,
                                                          std::max<size_t>(n + n / 8, 1u << 20)));
        const size_t rb = wide ? sizeof(RecW) : sizeof(RecC);
        const size_t padn = cap + kTileThreads;   // kernels write inactive lanes past n
        // (freed first: a batch that only turns wide may be sized below the last one)
        B.cap_n = 0;
        B.rec0.free(); B.rec1.free(); B.pos0.free(); B.pos1.free(); B.res.free(); B.tok.free();
        B.ext.free(); B.digit.free();
        int rc = B.rec0.reserve(padn * rb);
        if (rc == RL_OK) rc = B.digit.reserve(padn);
        if (rc == RL_OK) rc = B.rec1.reserve(padn * rb);
        if (rc == RL_OK) rc = B.pos0.reserve(padn);
        if (rc == RL_OK) rc = B.pos1.reserve(padn);
        if (rc == RL_OK) rc = B.res.reserve(padn);
        if (rc == RL_OK) rc = B.tok.reserve(padn);
        if (rc == RL_OK) rc = B.ext.reserve(padn);
        if (rc != RL_OK) return rc;
        B.cap_n = cap;
        B.cap_wide = wide;
    }
    if (counts_words <= B.counts.cap) return RL_OK;
    return B.counts.reserve(std::max(counts_words, (size_t)(1u << kMaxDigitBits) *
                                                       ((std::max<size_t>(n, B.cap_n) + kTile - 1) / kTile)));
}

// rstart / rend per region for two-pass partitions (k_group).
static int ensure_regions(BatchScratch& B, size_t bins) {
    const int rc = B.region_count.reserve(bins);
    return rc == RL_OK ? B.region_start.reserve(bins) : rc;
}

// chunk summaries [l1] then group summaries [l1 / 64 + kHotMax + 1], 64 B each (two keys)
static int ensure_hot_summ(rl_engine* e, size_t n) {
    const size_t l1 = n / kHotChunk + kHotMax + 1;
    const size_t need = l1 + l1 / 64 + kHotMax + 1;
    if (need * 8 <= e->hot_summ.cap) return RL_OK;
    if (e->hot_summ.reserve(need * 8) != RL_OK) return RL_E_NOMEM;
    e->hot_summ_l1 = l1;
    return RL_OK;
}

static int ensure_hot_mark(rl_engine* e, size_t bins) {
    if (bins <= e->hot_mark.cap) return RL_OK;
    if (e->hot_mark.reserve(bins) != RL_OK) return RL_E_NOMEM;
    HIP_OK(hipMemset(e->hot_mark, 0, bins * sizeof(uint32_t)));
    e->epoch = 0;
    return RL_OK;
}

static inline void mark_on(rl_engine* e, hipStream_t st, int i) {
    if (e->timing) (void)hipEventRecord(e->ev[e->ring_next][i], st);
}
static inline void mark(rl_engine* e, int i) { mark_on(e, e->stream, i); }

// ------------------------------------------------------------------ the small-batch path
// Who asks: a caller of the public entry points, the router for a batch of its own, the
// string-key call; `decided`: the host form chose before it staged anything.
enum class SmallAsk { decided, caller, router, keys };
static_assert(kSmallMax == RL_SMALL_BATCH_MAX, "rl_small.hpp and rl_engine.h agree");

// Whether this batch takes the path. A batch of eligible size (n <= rl_tune "small_batch")
// that does not is counted as declined; the reasons are the list of include/rl_engine.h.
static bool small_route(rl_engine* e, size_t n, SmallAsk who) {
    if (e->small_batch == 0 || n == 0 || n > e->small_batch) return false;
    bool wide = e->force_wide;
    for (auto& l : e->lims) wide |= l.cfg.max_permits > kCompactMaxPermits;
    if (n > kSmallMax || who != SmallAsk::caller || e->timing || e->pipeline || e->debug_regions ||
        e->lims.empty() || wide) {
        ++e->small_declined;
        return false;
    }
    return true;
}

static int ensure_small(rl_engine* e) {
    int rc = e->sm_rec.reserve(small_rec_count());
    if (rc == RL_OK) rc = e->sm_res.reserve(small_rec_count());
    if (rc == RL_OK) rc = e->sm_ext.reserve(small_rec_count());
    if (rc == RL_OK) rc = e->sm_tok.reserve(small_rec_count());
    if (rc == RL_OK) rc = e->sm_ctl.reserve(1);
    if (rc == RL_OK) rc = e->sm_stats.reserve(kStWords);
    // (indexed by region: they follow the tables' growth; growing frees, which waits for the device)
    if (rc == RL_OK) rc = e->sm_rstart.reserve(small_region_words(e->n_regions));
    if (rc == RL_OK) rc = e->sm_rend.reserve(small_region_words(e->n_regions));
    if (rc == RL_OK) rc = e->sm_order.reserve(small_order_words(e->n_regions));
    return rc;
}

// One launch on e->stream: the whole batch, its control block into h_ctl (mapped) by the kernel
// itself. The arrays are the caller's device arrays, or the host form's mapped block.
static int run_small(rl_engine* e, size_t n, const uint64_t* key, const int32_t* permits,
                     const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op,
                     uint8_t* allowed, int64_t* remaining, double* tokens_after) {
    const int rc = ensure_small(e);
    if (rc != RL_OK) return rc;
    SmallArgs a{};
    RegionArgs& ra = a.ra;
    ra.rec = e->sm_rec; ra.rstart = e->sm_rstart; ra.rend = e->sm_rend;
    ra.region_lim = e->d_region_lim; ra.lims = e->d_lims;
    ra.res = e->sm_res; ra.ext = e->sm_ext; ra.tok = e->sm_tok; ra.ctl = e->sm_ctl;
    ra.n_regions = e->n_regions; ra.n_total = (uint32_t)n; ra.shard_bits = e->shard_bits;
    ra.skew_ms = e->opts.max_skew_ms; ra.stats = e->sm_stats;
    for (auto& l : e->lims) ra.cache |= l.dev.cache_ttl_ms > 0 ? 1u : 0u;
    ra.sparse_max = e->sparse_max;
    ra.order = e->sm_order; ra.order_prefix = 0;
    a.key = key; a.permits = permits; a.now_ns = now_ns; a.limiter = limiter; a.op = op;
    a.allowed = allowed; a.remaining = remaining; a.tokens_out = tokens_after;
    a.rstart = e->sm_rstart; a.rend = e->sm_rend; a.order = e->sm_order;
    HIP_OK(hipHostGetDevicePointer((void**)&a.ctl_out, e->h_ctl, 0));
    a.n = (uint32_t)n; a.n_lim = (uint32_t)e->lims.size();
    e->last_wide = false;
    HIP_OK(launch_small_batch(a, e->stream));
    ++e->small_taken;
    e->last_small = true;
    e->pending_status = true;
    return RL_OK;
}

// The pipeline on device buffers, enqueued on e->stream. Returns an immediate status
// (argument/launch errors); the data-dependent status is read back by rl_last_status.
static int run_batch_device(rl_engine* e, size_t n, const uint64_t* key, const int32_t* permits,
                            const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op,
                            uint8_t* allowed, int64_t* remaining, double* tokens_after,
                            bool overlap = false, SmallAsk small = SmallAsk::decided) {
    if (n > e->opts.max_batch) return RL_E_TOO_LARGE;
    e->last_n = n;
    e->pending_status = false;
    e->enqueued = false;
    e->last_small = false;
    e->last_status = RL_OK;
    if (n == 0) return RL_OK;
    if (!key || !permits || !now_ns || !allowed || !remaining) return RL_E_INVALID_ARG;
    if (e->inject_fail) { --e->inject_fail; return RL_E_DEVICE; }   // nothing enqueued
    if (small != SmallAsk::decided && small_route(e, n, small))
        return run_small(e, n, key, permits, now_ns, limiter, op, allowed, remaining, tokens_after);
    hipStream_t s = e->stream;
    if (e->lims.empty()) {
        HIP_OK(launch_fill_invalid(allowed, remaining, tokens_after, (uint32_t)n, s));
        e->last_status = RL_E_INVALID_REQUEST;
        return RL_OK;
    }
    bool wide = e->force_wide;
    int64_t max_any = 0;
    for (auto& l : e->lims) {
        wide |= l.cfg.max_permits > kCompactMaxPermits;
        max_any = std::max<int64_t>(max_any, l.cfg.max_permits);
    }
    const int res_bytes = res_bytes_for(max_any, wide);
    bool cache = false;
    for (auto& l : e->lims) cache |= l.dev.cache_ttl_ms > 0;
    const uint32_t n_bins = e->n_regions;            // one partition bin per region
    BatchPlan P;
    int rc = plan_batch(e->tune, n, n_bins, &P);
    if (rc != RL_OK) return rc;
    const int passes = P.passes, dh = P.dh, s0 = P.s0;
    const uint32_t nt = P.nt, nb0 = P.nb0, n_segs = P.n_segs;
    const bool hot = P.hot, route = P.route;
    // Scratch set and partition stream. With RL_OPT_PIPELINE the partition (stages 1-3)
    // runs on e->pstream into one of two scratch sets, so batch k+1's partition overlaps
    // batch k's region stage; the region stage and the unpermute stay on e->stream (state
    // updates in batch order). `overlap`: the caller guarantees the inputs are complete
    // (device call with no stream); otherwise the partition first waits for everything
    // enqueued on e->stream (inputs copied or produced there, or the caller's stream).
    const int set = e->pipeline ? e->next_set : 0;
    BatchScratch& B = e->sc[set];
    uint32_t* r_list = e->route_list + (size_t)set * kRouteWords;
    uint32_t* r_start = e->route_start + (size_t)set * kRouteSlots;
    uint32_t* r_cnt = e->route_cnt + (size_t)set * kRouteSlots;
    hipStream_t ps = e->pipeline ? e->pstream : s;
    // Every buffer the chain is sized by, before anything is enqueued.
    const size_t region_words = passes == 2 ? n_bins : 0;
    if (e->pipeline && (!scratch_fits(B, n, wide) || P.counts_words > B.counts.cap ||
                        region_words > B.region_start.cap || P.seg_words > B.seg.cap ||
                        P.gtile_words > B.gtile.cap)) {
        // growing a set frees its old buffers: nothing may still be using them
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipStreamSynchronize(ps));
    }
    rc = ensure_scratch(e, B, n, wide, P.counts_words);
    if (rc == RL_OK) rc = ensure_regions(B, region_words);
    if (rc == RL_OK) rc = B.seg.reserve(P.seg_words);
    if (rc == RL_OK) rc = B.gtile.reserve(P.gtile_words);
    if (rc == RL_OK && e->debug_regions) rc = e->dbg.reserve((size_t)n_bins * kDbgWords);
    if (rc == RL_OK && e->region_order) rc = e->order.reserve((size_t)n_bins + 1);
    if (rc != RL_OK) return rc;
    if (e->pipeline) {
        if (B.used) HIP_OK(hipStreamWaitEvent(ps, B.freed, 0));    // the set's last batch is done
        if (!overlap) {
            HIP_OK(hipEventRecord(e->in_ev, s));
            HIP_OK(hipStreamWaitEvent(ps, e->in_ev, 0));
        }
    }
    if (hot) {
        rc = ensure_hot_mark(e, n_bins);
        if (rc == RL_OK) rc = ensure_hot_summ(e, n);
        if (rc != RL_OK) return rc;
        // Allow-walk tables (512 MiB): only once a batch had a key dense enough to walk
        // (k_hot_scan's count; a workload that never walks, such as tb_uniform, holds none).
        // The walk is optional and decides identically: a failed allocation turns it off.
        if (e->walk && !e->walk_tab && e->walk_hint > 0 && e->walk_tab.reserve(kWalkTabEntries) != RL_OK) {
            std::fprintf(stderr, "rl_engine: no device memory for the allow-walk tables; walks off\n");
            e->walk = false;
        }
        if (++e->epoch == 0) {                       // marks hold epochs: restart after wrap
            HIP_OK(hipMemsetAsync(e->hot_mark, 0, e->hot_mark.cap * sizeof(uint32_t), s));
            e->epoch = 1;
        }
    }
    e->last_wide = wide;

    mark_on(e, ps, 0);
    PartArgs pa{};
    pa.key = key; pa.permits = permits; pa.now_ns = now_ns; pa.limiter = limiter; pa.op = op;
    pa.n = (uint32_t)n; pa.n_tiles = nt; pa.tile_items = P.titems; pa.n_lim = (uint32_t)e->lims.size();
    pa.shard_bits = e->shard_bits; pa.lims = e->d_lims; pa.ctl = B.d_ctl;
    pa.counts = B.counts; pa.bin_base = B.bin_base; pa.ablate = e->ablate;
    pa.up_per_cu = P.up_per_cu;
    pa.sc_per_cu = e->sc_per_cu; pa.sc_split = e->sc_split;
    // ---- pass 0 (the high digit: region >> s0) from the caller's arrays; routed hot
    // regions get bins 2^dh + slot and their records go straight to the final array (rec1)
    pa.digit_shift = s0; pa.digit_bits = P.digit_bits;
    pa.n_bins_pass = nb0;
    pa.rec_out = passes == 2 ? B.rec0 : B.rec1; pa.pos_out = B.pos0;
    if (route) {
        pa.route_list = r_list; pa.lo_bins = 1u << dh; pa.rec_out_route = B.rec1;
        pa.digit = B.digit;
    }
    HIP_OK(launch_upsweep(pa, ps));
    mark_on(e, ps, 1);
    HIP_OK(launch_scan_rows(B.counts, B.counts, nb0, nt, B.bin_total, ps));
    HIP_OK(launch_scan_small(B.bin_total, B.bin_base, nb0, ps));
    if (n_segs > 1) {
        const size_t m = (size_t)nb0 * n_segs;
        HIP_OK(launch_seg_base(B.counts, B.bin_total, B.bin_base, nb0, 1u << dh, nt, P.seg_tiles, n_segs,
                               B.seg, B.seg + m, B.seg + 2 * m, ps));
        pa.seg_adj = B.seg; pa.n_segs = n_segs; pa.seg_tiles = P.seg_tiles;
    }
    mark_on(e, ps, 2);
    HIP_OK(launch_scatter(pa, wide, ps));
    if (route)
        HIP_OK(launch_route_ranges(r_list, B.bin_base, B.bin_total, 1u << dh, r_start, r_cnt,
                                   B.d_ctl, ps));
    mark_on(e, ps, 3);
    const void* rec_final = B.rec1;
    const uint32_t* rstart = B.bin_base;
    const uint32_t* rcount = B.bin_total;
    const uint32_t* rend = nullptr;
    if (passes == 2) {
        // ---- each normal pass-0 bin grouped by region in its own range of the final array
        // (stable: arrival order inside each region); the regions' bounds and the pass-0 ->
        // final positions (pos1) come with it. Routed records stay where pass 0 put them.
        GroupArgs ga{};
        ga.rec_in = B.rec0; ga.rec_out = B.rec1; ga.pos_out = B.pos1;
        ga.bin_base = B.bin_base; ga.bin_total = B.bin_total;
        ga.rstart = B.region_start; ga.rend = B.region_count;
        ga.lims = e->d_lims; ga.n_lim = (uint32_t)e->lims.size(); ga.shard_bits = e->shard_bits;
        ga.n_bins0 = 1u << dh; ga.sub_bits = (uint32_t)s0; ga.n_regions = n_bins;
        ga.tile_recs = P.tile_recs; ga.max_tiles = P.max_tiles;
        ga.pad = (uint32_t)n;
        ga.ablate = e->ablate;
        // B.gtile (P.gtile_words): tile_base, tile_bin, tcount, then tile_beg / tile_end
        ga.tile_base = B.gtile;
        ga.tile_bin = B.gtile + ga.n_bins0 + 1;
        ga.tcount = ga.tile_bin + ga.max_tiles;
        if (n_segs > 1) {
            const size_t m = (size_t)nb0 * n_segs;
            ga.seg_start = B.seg + m; ga.seg_cnt = B.seg + 2 * m; ga.n_segs = n_segs;
            ga.tile_beg = ga.tcount + (size_t)ga.max_tiles * ((size_t)1 << s0);
            ga.tile_end = ga.tile_beg + ga.max_tiles;
        }
        HIP_OK(launch_group(ga, wide, ps));
        rstart = B.region_start;
        rcount = nullptr;
        rend = B.region_count;
    }
    mark_on(e, ps, 4);
    mark_on(e, ps, 5);
    mark_on(e, ps, 6);
    if (e->pipeline) {
        HIP_OK(hipEventRecord(B.parted, ps));
        HIP_OK(hipStreamWaitEvent(s, B.parted, 0));
    }
    RegionArgs ra{};
    ra.rec = rec_final; ra.rstart = rstart; ra.rcount = rcount; ra.rend = rend;
    ra.region_lim = e->d_region_lim;
    ra.lims = e->d_lims; ra.res = B.res; ra.ext = B.ext; ra.tok = tokens_after ? B.tok : nullptr;
    ra.ctl = B.d_ctl; ra.n_regions = e->n_regions; ra.n_total = (uint32_t)n; ra.ablate = e->ablate;
    ra.shard_bits = e->shard_bits;
    ra.skew_ms = e->opts.max_skew_ms;
    ra.stats = e->d_stats;
    ra.cache = cache ? 1u : 0u;
    ra.sparse_max = e->sparse_max;
    // chain launch size: twice the hot count of the last batch the host saw complete (a
    // hint only: the chains loop over the hot list with the grid's stride), the whole
    // kHotMax before any batch has completed
    ra.chain_split = e->chain_split ? 1u : 0u;
    if (e->hot_hint != 0xFFFFFFFFu) {
        const uint32_t nh = e->hot_hint;
        ra.chain_grid = nh ? std::min<uint32_t>(kHotMax, std::max<uint32_t>(256u, 2u * nh)) : 64u;
    }
    if (e->debug_regions) {
        HIP_OK(hipMemsetAsync(e->dbg, 0, e->dbg.cap * sizeof(uint64_t), s));
        ra.dbg = e->dbg;
    }
    if (hot) {
        uint32_t* hot_count = e->hot_list + kHotMax;
        HIP_OK(hipMemsetAsync(hot_count, 0, kHotMetaWords * sizeof(uint32_t), s));
        if (route) HIP_OK(launch_hot_route_list(r_list, r_cnt, e->hot_list, hot_count, s));
        HIP_OK(launch_hot_select(rstart, rcount, rend, n_bins, P.hot_thr, e->hot_list,
                                 hot_count, e->hot_mark, e->epoch, cache ? e->d_lims : nullptr,
                                 e->d_region_lim, s));
        ra.hot_list = e->hot_list; ra.hot_count = hot_count; ra.hot_mark = e->hot_mark;
        ra.epoch = e->epoch;
        ra.hot_info = e->hot_info; ra.hot_summ = e->hot_summ;
        ra.hot_summ2 = e->hot_summ + e->hot_summ_l1 * 8; ra.hot_total = e->hot_list + kHotMax + kHotTotalOff;
        ra.route_list = r_list; ra.route_start = r_start; ra.route_cnt = r_cnt;
        ra.walk_tab = e->walk ? e->walk_tab : nullptr;
        ra.walk_min = e->walk_min;
        HIP_OK(launch_hot_prepare(ra, wide, s));          // dominant keys, chunk summaries
        HIP_OK(launch_chains(ra, wide, res_bytes, s, e->hstream, e->hot_ev[0]));
        // the chains' decided chunks filled on the side stream as soon as the chains end,
        // beside the normal regions' tail (sw_zipf: chains ~2.8 ms, normal drain ~3.3 ms)
        HIP_OK(launch_hot_fill(ra, wide, res_bytes, e->hstream));
    }
    if (e->region_order) {
        HIP_OK(launch_region_order(rstart, rcount, rend, n_bins, e->order_meta, e->order, s));
        ra.order = e->order;
        ra.order_prefix = e->order_prefix;
    }
    if (cache && e->solo_threshold) {
        // cache-on sliding windows have no hot path: a key's leading allow run in a large
        // region is decided by a whole workgroup, the rest by its region wave (rl_solo.hip).
        // (k_solo_select lists cache-on regions only, which k_hot_select never lists.)
        uint32_t* cnt = e->solo_list + kSoloMax;
        HIP_OK(hipMemsetAsync(cnt, 0, sizeof(uint32_t), s));
        HIP_OK(launch_solo_select(rstart, rcount, rend, n_bins, e->solo_threshold, e->d_lims,
                                  e->d_region_lim, e->solo_list, cnt, s));
        HIP_OK(launch_solo(ra, wide, res_bytes, (uint32_t*)rstart, (uint32_t*)rcount, e->solo_list, cnt, s));
    }
    mark(e, 7);
    // the regions (the hot chains run on the side stream since launch_chains)
    HIP_OK(launch_region(ra, wide, res_bytes, s, hot ? e->hstream : nullptr, e->hot_ev[1]));
    mark(e, 10);
    // (hot: the fill ran on the side stream, joined by launch_region)
    // the next batch's routed regions: this batch's largest hot regions (two-pass tables)
    if (hot && e->tune.route && passes == 2)
        HIP_OK(launch_route_next(e->hot_info, e->hot_list + kHotMax, P.hot_thr, r_list, s));
    HIP_OK(launch_stats_reduce(e->d_stats, B.d_ctl, s));
    mark(e, 11);
    mark(e, 8);
    UnpermArgs ua{};
    ua.pos0 = B.pos0; ua.pos1 = passes == 2 ? B.pos1 : nullptr; ua.res = B.res;
    ua.mid = B.rec0;                                    // pass-0 records are dead by now
    ua.tok = tokens_after ? B.tok : nullptr;
    ua.ext = B.ext; ua.ctl = B.d_ctl;
    ua.allowed = allowed; ua.remaining = remaining; ua.tokens_out = tokens_after;
    ua.n = (uint32_t)n; ua.n_tiles = P.nt_un; ua.ablate = e->ablate; ua.per_cu = e->un_per_cu;
    ua.split = e->un_split == 1 || (e->un_split == 2 && passes == 2);
    ua.mid_xcd = e->mid_xcd;
    HIP_OK(launch_unpermute(ua, res_bytes, s));
    mark(e, 9);
    if (e->timing) {
        e->ring_next = (e->ring_next + 1) % kEvRing;
        e->ring_used = std::min(e->ring_used + 1, kEvRing);
    }
    HIP_OK(hipMemcpyAsync(e->h_ctl, B.d_ctl, sizeof(BatchCtl), hipMemcpyDeviceToHost, s));
    if (e->pipeline) {
        HIP_OK(hipEventRecord(B.freed, s));
        B.used = true;
        e->next_set ^= 1;
    }
    e->pending_status = true;
    e->enqueued = true;
    return RL_OK;
}

// on-demand growth: a limiter whose regions are filling up (or overflowed: then twice)
// gets twice (four times) the regions before the next batch
static void apply_growth(rl_engine* e, const unsigned long long (&grow)[4], bool overflowed) {
    if (!e->auto_grow || !(grow[0] | grow[1] | grow[2] | grow[3])) return;
    for (size_t li = 0; li < e->lims.size(); ++li) {
        if (!((grow[li >> 6] >> (li & 63)) & 1ULL)) continue;
        for (int t = 0; t < (overflowed ? 2 : 1); ++t)
            if (grow_once(e, li) != RL_OK) break;          // at the table-size limit: stay
    }
}

static int status_of(bool invalid, bool cap_err, bool span_overflow, bool internal) {
    int st = RL_OK;
    if (invalid) st = RL_E_INVALID_REQUEST;
    if (cap_err) st = RL_E_CAPACITY;
    if (span_overflow) st = RL_E_INVALID_ARG;
    if (internal) st = RL_E_INTERNAL;
    return st;
}

int collect_status(rl_engine* e) {
    HIP_OK(hipStreamSynchronize(e->stream));
    if (e->pstream) HIP_OK(hipStreamSynchronize(e->pstream));
    if (!e->pending_status) return e->last_status;
    e->pending_status = false;
    BatchCtl& c = *e->h_ctl;
    if (!e->last_small) {                            // (a small batch says nothing about hot regions)
        e->hot_hint = c.n_hot;
        e->walk_hint = c.n_walk;
    }
    const int st = status_of(c.invalid != 0, c.cap_err != 0, c.span_overflow != 0, c.internal_err != 0);
    e->last_status = st;
    apply_growth(e, c.grow, c.cap_err != 0);
    c.grow[0] = c.grow[1] = c.grow[2] = c.grow[3] = 0;
    return st;
}

namespace rl {
int engine_status_accum(rl_engine* e, unsigned long long* acc, void* stream) {
    if (!e || !acc) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    const BatchScratch& B = e->sc[e->pipeline ? e->next_set ^ 1 : 0];   // the last batch's set
    // A call that enqueued no batch (nothing received in this round, or a status set on the
    // host) leaves d_ctl holding an earlier batch whose status and growth were already
    // applied: fold only the host-side status then.
    const unsigned long long host = e->last_status == RL_E_INVALID_REQUEST ? 1ULL : 0ULL;
    HIP_OK(launch_status_accum(e->enqueued ? B.d_ctl : nullptr, e->enqueued ? 0ULL : host, acc,
                               stream ? (hipStream_t)stream : e->stream));
    return RL_OK;
}

int engine_status_settle(rl_engine* e, const unsigned long long* acc) {
    if (!e || !acc) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_OK(hipStreamSynchronize(e->stream));
    if (e->pstream) HIP_OK(hipStreamSynchronize(e->pstream));
    // the last batch's own status is part of acc: it must not be collected (grown) again
    e->pending_status = false;
    if (e->enqueued) { e->hot_hint = e->h_ctl->n_hot; e->walk_hint = e->h_ctl->n_walk; }
    const int st = status_of(acc[0] & 1u, acc[0] & 2u, acc[0] & 4u, acc[0] & 8u);
    e->last_status = st;
    const unsigned long long grow[4] = {acc[1], acc[2], acc[3], acc[4]};
    apply_growth(e, grow, (acc[0] & 2u) != 0);
    return st;
}
}  // namespace rl

static int execute_device(rl_engine* e, size_t n, const uint64_t* key, const int32_t* permits,
                          const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op,
                          uint8_t* allowed, int64_t* remaining, double* tokens_after, void* stream,
                          SmallAsk who) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    StreamJoin join(e->stream, (hipStream_t)stream);
    HIP_OK(join.err);
    const int rc = run_batch_device(e, n, key, permits, now_ns, limiter, op, allowed, remaining,
                                    tokens_after, /*overlap=*/stream == nullptr, who);
    HIP_OK(join.finish());
    return rc;
}

extern "C" int rl_execute_batch_device(rl_engine* e, size_t n, const uint64_t* key,
                                       const int32_t* permits, const int64_t* now_ns,
                                       const uint16_t* limiter, const uint8_t* op,
                                       uint8_t* allowed, int64_t* remaining, double* tokens_after,
                                       void* stream) {
    return execute_device(e, n, key, permits, now_ns, limiter, op, allowed, remaining, tokens_after,
                          stream, SmallAsk::caller);
}

namespace rl {
int engine_execute_routed(rl_engine* e, size_t n, const uint64_t* key, const int32_t* permits,
                          const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op,
                          uint8_t* allowed, int64_t* remaining, double* tokens_after, void* stream) {
    return execute_device(e, n, key, permits, now_ns, limiter, op, allowed, remaining, tokens_after,
                          stream, SmallAsk::router);
}
}  // namespace rl

extern "C" int rl_small_batches(rl_engine* e, uint64_t* taken, uint64_t* declined) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (taken) *taken = e->small_taken;
    if (declined) *declined = e->small_declined;
    return RL_OK;
}

// The string-key call stages and hashes on the device: always the pipeline (counted as declined).
void small_decline_keys(rl_engine* e, size_t n) { (void)small_route(e, n, SmallAsk::keys); }

extern "C" int rl_last_status(rl_engine* e) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return collect_status(e);
}

int ensure_staging(rl_engine* e, size_t n) {
    int rc = e->s_key.reserve(n);
    if (rc == RL_OK) rc = e->s_permits.reserve(n);
    if (rc == RL_OK) rc = e->s_now.reserve(n);
    if (rc == RL_OK) rc = e->s_lim.reserve(n);
    if (rc == RL_OK) rc = e->s_op.reserve(n);
    if (rc == RL_OK) rc = e->s_allowed.reserve(n);
    if (rc == RL_OK) rc = e->s_remaining.reserve(n);
    if (rc == RL_OK) rc = e->s_tokens.reserve(n);
    return rc;
}

// The host-buffer calls' requests into the staging arrays (limiter, op_or_skip: nullable; key
// null: s_key is filled by the caller, rl_execute_batch_keys; permits null: rl_quota without them).
int stage_requests(rl_engine* e, size_t n, const uint64_t* key, const int32_t* permits,
                   const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op_or_skip) {
    const int rc = ensure_staging(e, n);
    if (rc != RL_OK) return rc;
    hipStream_t s = e->stream;
    if (key) HIP_OK(hipMemcpyAsync(e->s_key, key, n * 8, hipMemcpyHostToDevice, s));
    if (permits) HIP_OK(hipMemcpyAsync(e->s_permits, permits, n * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(e->s_now, now_ns, n * 8, hipMemcpyHostToDevice, s));
    if (limiter) HIP_OK(hipMemcpyAsync(e->s_lim, limiter, n * 2, hipMemcpyHostToDevice, s));
    if (op_or_skip) HIP_OK(hipMemcpyAsync(e->s_op, op_or_skip, n, hipMemcpyHostToDevice, s));
    return RL_OK;
}

// The staged batch (stage_requests) run, collected and copied back: the body of the host-buffer
// batch calls.
int run_staged_batch(rl_engine* e, size_t n, bool limiter, bool op, uint8_t* allowed,
                     int64_t* remaining, double* tokens_after) {
    hipStream_t s = e->stream;
    auto run = [&] {
        return run_batch_device(e, n, e->s_key, e->s_permits, e->s_now, limiter ? e->s_lim.p : nullptr,
                                op ? e->s_op.p : nullptr, e->s_allowed, e->s_remaining,
                                tokens_after ? e->s_tokens.p : nullptr);
    };
    int rc = run();
    if (rc != RL_OK) { (void)hipStreamSynchronize(s); return rc; }
    rc = collect_status(e);
    if (rc == RL_E_INVALID_ARG && e->h_ctl->span_overflow && !e->force_wide) {
        // the batch spans more than the compact record's 2^32 ms: it was rejected before any
        // state was touched, so run it again in 32-B records (full now_ms)
        e->force_wide = true;
        rc = run();
        e->force_wide = false;
        if (rc != RL_OK) { (void)hipStreamSynchronize(s); return rc; }
        rc = collect_status(e);
    }
    HIP_OK(hipMemcpyAsync(allowed, e->s_allowed, n, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(remaining, e->s_remaining, n * 8, hipMemcpyDeviceToHost, s));
    if (tokens_after) HIP_OK(hipMemcpyAsync(tokens_after, e->s_tokens, n * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return rc;
}

// The host form of the small-batch path: the requests packed into the engine's page-locked
// block, which the kernel reads and writes in place (mapped), one synchronisation, the results
// copied out. A batch whose span the compact records cannot hold was rejected before any state
// was touched: it goes to the pipeline in 32-B records, as run_staged_batch's retry does.
static int run_small_host(rl_engine* e, size_t n, const uint64_t* key, const int32_t* permits,
                          const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op,
                          uint8_t* allowed, int64_t* remaining, double* tokens_after) {
    e->last_n = n;
    e->pending_status = false;
    e->enqueued = false;
    e->last_small = false;
    e->last_status = RL_OK;
    if (e->inject_fail) { --e->inject_fail; return RL_E_DEVICE; }
    const SmallBlock b = small_block();
    if (!e->sm_block && hipHostMalloc((void**)&e->sm_block, b.bytes) != hipSuccess) {
        e->sm_block = nullptr;
        return RL_E_NOMEM;
    }
    uint8_t* h = e->sm_block;
    uint8_t* d = nullptr;
    HIP_OK(hipHostGetDevicePointer((void**)&d, h, 0));
    std::memcpy(h + b.key, key, n * 8);
    std::memcpy(h + b.now_ns, now_ns, n * 8);
    std::memcpy(h + b.permits, permits, n * 4);
    if (limiter) std::memcpy(h + b.limiter, limiter, n * 2);
    if (op) std::memcpy(h + b.op, op, n);
    int rc = run_small(e, n, (const uint64_t*)(d + b.key), (const int32_t*)(d + b.permits),
                       (const int64_t*)(d + b.now_ns), limiter ? (const uint16_t*)(d + b.limiter) : nullptr,
                       op ? d + b.op : nullptr, d + b.allowed, (int64_t*)(d + b.remaining),
                       tokens_after ? (double*)(d + b.tokens) : nullptr);
    if (rc != RL_OK) { (void)hipStreamSynchronize(e->stream); return rc; }
    rc = collect_status(e);
    if (rc == RL_E_INVALID_ARG && e->h_ctl->span_overflow) {
        ++e->small_declined;                          // (wide records: the pipeline's)
        e->force_wide = true;                         // (small_route declined a force_wide engine)
        rc = stage_requests(e, n, key, permits, now_ns, limiter, op);
        if (rc == RL_OK)
            rc = run_staged_batch(e, n, limiter != nullptr, op != nullptr, allowed, remaining, tokens_after);
        e->force_wide = false;
        return rc;
    }
    std::memcpy(allowed, h + b.allowed, n);
    std::memcpy(remaining, h + b.remaining, n * 8);
    if (tokens_after) std::memcpy(tokens_after, h + b.tokens, n * 8);
    return rc;
}

extern "C" int rl_execute_batch(rl_engine* e, size_t n, const uint64_t* key,
                                const int32_t* permits, const int64_t* now_ns,
                                const uint16_t* limiter, const uint8_t* op, uint8_t* allowed,
                                int64_t* remaining, double* tokens_after) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (n > e->opts.max_batch) return RL_E_TOO_LARGE;
    if (n == 0) return RL_OK;
    if (!key || !permits || !now_ns || !allowed || !remaining) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    if (small_route(e, n, SmallAsk::caller))
        return run_small_host(e, n, key, permits, now_ns, limiter, op, allowed, remaining, tokens_after);
    int rc = stage_requests(e, n, key, permits, now_ns, limiter, op);
    if (rc != RL_OK) return rc;
    return run_staged_batch(e, n, limiter != nullptr, op != nullptr, allowed, remaining, tokens_after);
}

extern "C" int rl_try_acquire_batch(rl_engine* e, size_t n, const uint64_t* key_hash,
                                    const int32_t* permits, const int64_t* now_ns,
                                    const uint16_t* limiter, uint8_t* allowed, int64_t* remaining,
                                    double* tokens_after) {
    return rl_execute_batch(e, n, key_hash, permits, now_ns, limiter, nullptr, allowed, remaining,
                            tokens_after);
}

static int admin_op(rl_engine* e, uint16_t limiter, size_t n, const uint64_t* key,
                    const int64_t* now_ns, uint8_t opcode, int64_t* out) {
    if (!e || (n && (!key || !now_ns))) return RL_E_INVALID_ARG;
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    if (n == 0) return RL_OK;
    std::vector<int32_t> p(n, 1);
    std::vector<uint16_t> l(n, limiter);
    std::vector<uint8_t> o(n, opcode), a(n);
    std::vector<int64_t> r(n);
    int rc = rl_execute_batch(e, n, key, p.data(), now_ns, l.data(), o.data(), a.data(), r.data(),
                              nullptr);
    if (out) std::memcpy(out, r.data(), n * sizeof(int64_t));
    return rc;
}

extern "C" int rl_available(rl_engine* e, uint16_t limiter, size_t n, const uint64_t* key_hash,
                            const int64_t* now_ns, int64_t* available) {
    if (!available && n) return RL_E_INVALID_ARG;
    return admin_op(e, limiter, n, key_hash, now_ns, RL_OP_PEEK, available);
}

extern "C" int rl_reset(rl_engine* e, uint16_t limiter, size_t n, const uint64_t* key_hash,
                        const int64_t* now_ns) {
    return admin_op(e, limiter, n, key_hash, now_ns, RL_OP_RESET, nullptr);
}
