// rl_engine_state.cpp — a table's contents moved as a whole: state export and import, key
// migration (copy, drop, put), snapshot and restore, the sweep and the table shrink.
#include "rl_engine_impl.hpp"
#include "rl_shrink.hpp"
#include "rl_snapshot.hpp"

using namespace rl;

// ---------------------------------------------------------------- state export / import
// the engine's state in the reference's Redis keyspace layout
// (SlidingWindowRateLimiter.java:185-188 + RedisRateLimitStorage.java:38-49;
// TokenBucketRateLimiter.java:46-48,63-64).
static_assert(sizeof(StateRec) == sizeof(rl_state_entry), "StateRec layout");
static_assert(offsetof(StateRec, expire_at_ms) == offsetof(rl_state_entry, expire_at_ms), "StateRec layout");

extern "C" int rl_export_state(rl_engine* e, int64_t now_ns, rl_state_entry* out, size_t cap,
                               size_t* n_out) {
    if (!e || !n_out || (cap && !out)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    const int64_t now = floor_div_ms(now_ns);
    const uint32_t dcap = (uint32_t)std::min<size_t>(cap, 0xFFFFFFF0u);
    DevArray<StateRec> d_out;
    DevArray<uint32_t> d_count;
    if (d_out.reserve(std::max<uint32_t>(dcap, 1u)) != RL_OK || d_count.reserve(1) != RL_OK) return RL_E_NOMEM;
    uint32_t total = 0;
    HIP_OK(hipMemsetAsync(d_count, 0, sizeof(uint32_t), e->stream));
    for (size_t li = 0; li < e->lims.size(); ++li) {
        const HostLimiter& h = e->lims[li];
        HIP_OK(launch_export((const Slot*)h.table, h.table_bytes / sizeof(Slot), h.dev, (uint16_t)li,
                             now, d_out, dcap, d_count, e->stream));
    }
    HIP_OK(hipMemcpyAsync(&total, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    *n_out = total;
    if (total > cap) return RL_E_TOO_LARGE;
    if (total == 0) return RL_OK;
    HIP_OK(hipMemcpy(out, d_out, (size_t)total * sizeof(StateRec), hipMemcpyDeviceToHost));
    std::sort(out, out + total, [](const rl_state_entry& x, const rl_state_entry& y) {
        if (x.limiter != y.limiter) return x.limiter < y.limiter;
        if (x.key_hash != y.key_hash) return x.key_hash < y.key_hash;
        return x.window_start_ms < y.window_start_ms;
    });
    return RL_OK;
}

// A slot image bound for the region at `addr` (its local-cache words at `xaddr`, 0: none), and
// the rebuild of every region that receives some (k_import), shared by rl_import_state and
// rl_put_keys: images in `imgs` order per region, `with_x` = carry their cache words (the state
// import writes 0). *fail = images that found no free slot. Synchronises the engine stream.
namespace {
struct RegionImg { uint64_t addr, xaddr; uint8_t algo; Slot s; uint64_t x; };

RegionImg region_img(const rl_engine* e, const HostLimiter& h, uint64_t tag) {
    RegionImg im{};
    const size_t slot0 = region_slot0(tag, e->shard_bits, h.dev.region_bits);
    im.algo = (uint8_t)h.dev.algo;
    im.s.tag = tag;
    im.addr = (uint64_t)(uintptr_t)((Slot*)h.table + slot0);
    im.xaddr = h.cache_table ? (uint64_t)(uintptr_t)((uint64_t*)h.cache_table + slot0) : 0;
    return im;
}

int apply_region_images(rl_engine* e, std::vector<RegionImg>& imgs, bool with_x, uint32_t* fail_out) {
    *fail_out = 0;
    if (imgs.empty()) return RL_OK;
    std::stable_sort(imgs.begin(), imgs.end(),
                     [](const RegionImg& x, const RegionImg& y) { return x.addr < y.addr; });
    std::vector<uint32_t> off;
    std::vector<uint64_t> addr, xaddr, xw(imgs.size());
    std::vector<uint8_t> algo;
    std::vector<Slot> slots(imgs.size());
    for (size_t k = 0; k < imgs.size(); ++k) {
        if (k == 0 || imgs[k].addr != imgs[k - 1].addr) {
            off.push_back((uint32_t)k);
            addr.push_back(imgs[k].addr);
            xaddr.push_back(imgs[k].xaddr);
            algo.push_back(imgs[k].algo);
        }
        slots[k] = imgs[k].s;
        xw[k] = imgs[k].x;
    }
    off.push_back((uint32_t)imgs.size());
    const size_t G = addr.size(), N = slots.size();
    const size_t bytes = N * sizeof(Slot) + N * 8 + G * 16 + (G + 1) * 4 + G + 16;
    DevArray<uint8_t> d;
    if (d.reserve(bytes) != RL_OK) return RL_E_NOMEM;
    Slot* d_img = (Slot*)d.p;
    uint64_t* d_xw = (uint64_t*)(d.p + N * sizeof(Slot));
    uint64_t* d_addr = d_xw + N;
    uint64_t* d_xaddr = d_addr + G;
    uint32_t* d_off = (uint32_t*)(d_xaddr + G);
    uint32_t* d_fail = d_off + G + 1;
    uint8_t* d_algo = (uint8_t*)(d_fail + 1);
    hipStream_t s = e->stream;
    HIP_OK(hipMemcpyAsync(d_img, slots.data(), N * sizeof(Slot), hipMemcpyHostToDevice, s));
    if (with_x) HIP_OK(hipMemcpyAsync(d_xw, xw.data(), N * 8, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(d_addr, addr.data(), G * 8, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(d_xaddr, xaddr.data(), G * 8, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(d_off, off.data(), (G + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(d_algo, algo.data(), G, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemsetAsync(d_fail, 0, 4, s));
    ImportArgs a{};
    a.n_groups = (uint32_t)G; a.group_off = d_off; a.region_addr = d_addr; a.xregion_addr = d_xaddr;
    a.group_algo = d_algo;
    a.img = d_img; a.xw = with_x ? d_xw : nullptr; a.fail = d_fail;
    HIP_OK(launch_import(a, s));
    HIP_OK(hipMemcpyAsync(fail_out, d_fail, 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return RL_OK;
}
}  // namespace

extern "C" int rl_import_state(rl_engine* e, const rl_state_entry* in, size_t n, size_t* n_imported) {
    if (!e || (n && !in)) return RL_E_INVALID_ARG;
    if (n_imported) *n_imported = 0;
    if (n == 0) return RL_OK;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    std::vector<const rl_state_entry*> v(n);
    for (size_t i = 0; i < n; ++i) {
        const rl_state_entry& x = in[i];
        if (x.limiter >= e->lims.size()) return RL_E_INVALID_ARG;
        const DevLimiter& L = e->lims[x.limiter].dev;
        if (x.kind != (L.algo == kAlgoTB ? RL_STATE_TB_BUCKET : RL_STATE_SW_BUCKET)) return RL_E_INVALID_ARG;
        if (L.algo == kAlgoTB) {
            if (x.expire_at_ms != x.last_refill_ms + L.ttl_ms) return RL_E_INVALID_ARG;
        } else {
            const int64_t w = L.window_ms;
            if (x.count < 1 || x.count > 0xFFFFFFFFLL || x.window_start_ms % w != 0) return RL_E_INVALID_ARG;
            const int64_t off = x.expire_at_ms - w - x.window_start_ms;   // last INCR - W
            if (off < 0 || off >= w) return RL_E_INVALID_ARG;
        }
        v[i] = &x;
    }
    // (limiter, key) groups, newest bucket first
    std::sort(v.begin(), v.end(), [](const rl_state_entry* x, const rl_state_entry* y) {
        if (x->limiter != y->limiter) return x->limiter < y->limiter;
        if (x->key_hash != y->key_hash) return x->key_hash < y->key_hash;
        return x->window_start_ms > y->window_start_ms;
    });
    std::vector<RegionImg> imgs;
    size_t taken = 0;
    for (size_t i = 0; i < n;) {
        size_t j = i + 1;
        while (j < n && v[j]->limiter == v[i]->limiter && v[j]->key_hash == v[i]->key_hash) ++j;
        const rl_state_entry& x = *v[i];
        const HostLimiter& h = e->lims[x.limiter];
        const DevLimiter& L = h.dev;
        const uint64_t tag = mix64(x.key_hash);
        const bool mine = e->opts.shard_count <= 1 ||
                          (uint32_t)(tag >> (64 - e->shard_bits)) == e->opts.shard_index;
        if (mine) {
            RegionImg im = region_img(e, h, tag);
            if (L.algo == kAlgoTB) {                  // one hash per key: the first one wins
                uint64_t bits;
                std::memcpy(&bits, &x.tokens, 8);
                im.s.a = bits; im.s.b = (uint64_t)x.last_refill_ms; im.s.c = 1;
                taken += 1;
            } else {
                const int64_t w = L.window_ms;
                int64_t b1 = x.window_start_ms;
                uint64_t c1 = (uint64_t)x.count, c0 = 0;
                int64_t o1 = x.expire_at_ms - w - b1, o0 = 0;
                taken += 1;
                if (j > i + 1 && v[i + 1]->window_start_ms == b1 - w) {
                    c0 = (uint64_t)v[i + 1]->count;
                    o0 = v[i + 1]->expire_at_ms - w - (b1 - w);
                    taken += 1;
                }
                im.s.a = (uint64_t)b1;
                im.s.b = c1 | (c0 << 32);
                im.s.c = (uint64_t)(uint32_t)o1 | ((uint64_t)(uint32_t)o0 << 32);
            }
            imgs.push_back(im);
        }
        i = j;
    }
    if (imgs.empty()) return RL_OK;
    uint32_t fail = 0;
    const int rc = apply_region_images(e, imgs, /*with_x=*/false, &fail);
    if (rc != RL_OK) return rc;
    if (n_imported) *n_imported = taken;
    return fail ? RL_E_CAPACITY : RL_OK;
}

// ---------------------------------------------------------------- key migration
// rl_copy_keys / rl_drop_keys / rl_put_keys (rl_migrate.hip, k_import). Like the census they run
// on the engine stream behind every batch submitted before them (the decision stage and the
// unpermute run on or are joined on e->stream, with RL_OPT_PIPELINE too), work on the table as
// installed (no collect_status) and touch no batch scratch, d_stats, d_ctl or status word.
// The slot and its cache word are a key's whole state between batches: the hot-region route
// list holds region ids chosen from the previous batch's record counts, the hot, walk and solo
// lists and the escape arrays are rebuilt from each batch's own records, and hot_hint /
// walk_hint only size scratch. None of them names a key or caches a slot's contents, so a put or
// a drop between two batches needs to invalidate nothing.
static_assert(sizeof(KeyImage) == sizeof(rl_key_image) && sizeof(rl_key_image) == 48, "rl_key_image layout");
static_assert(offsetof(KeyImage, limiter) == offsetof(rl_key_image, limiter), "rl_key_image layout");
static_assert(RL_MOVE_KEYS_MAX == kMoveKeysMax && RL_MOVE_KEYS_MAX >= 2 * kDirMax, "old + new directory");

// Copy (out / cap) or drop (out = nullptr) of the listed keys under every limiter; *count =
// the hits. Drop: key_hash 0 in a launch of its own (rl_migrate.hip).
static int move_keys(rl_engine* e, size_t n, const uint64_t* key_hash, bool drop, rl_key_image* out,
                     size_t cap, uint32_t* count) {
    *count = 0;
    std::vector<uint64_t> keys(key_hash, key_hash + n);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const size_t nk = keys.size(), n_lim = e->lims.size();
    if (nk == 0 || n_lim == 0) return RL_OK;
    const uint32_t dcap = drop ? 0u : (uint32_t)std::min<size_t>(cap, nk * n_lim);
    DevArray<uint64_t> d_keys;
    DevArray<KeyImage> d_out;
    DevArray<uint32_t> d_count;
    if (d_keys.reserve(nk) != RL_OK || d_out.reserve(std::max<uint32_t>(dcap, 1u)) != RL_OK ||
        d_count.reserve(1) != RL_OK)
        return RL_E_NOMEM;
    hipStream_t s = e->stream;
    HIP_OK(hipMemcpyAsync(d_keys, keys.data(), nk * 8, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemsetAsync(d_count, 0, sizeof(uint32_t), s));
    MoveArgs a{};
    a.key = d_keys; a.lims = e->d_lims; a.out = d_out; a.count = d_count;
    a.n_keys = (uint32_t)nk; a.n_lim = (uint32_t)n_lim; a.cap = dcap; a.shard_bits = e->shard_bits;
    if (drop && keys[0] == 0) {                          // (sorted: key 0 comes first)
        MoveArgs z = a;
        z.n_keys = 1;
        a.key = d_keys + 1; a.n_keys = (uint32_t)nk - 1;
        HIP_OK(launch_move_keys(a, true, s));
        HIP_OK(launch_move_keys(z, true, s));
    } else {
        HIP_OK(launch_move_keys(a, drop, s));
    }
    HIP_OK(hipMemcpyAsync(count, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (drop || *count == 0 || *count > cap) return RL_OK;
    if (*count > dcap) return RL_E_INTERNAL;             // (more hits than pairs)
    HIP_OK(hipMemcpy(out, d_out, (size_t)*count * sizeof(KeyImage), hipMemcpyDeviceToHost));
    std::sort(out, out + *count, [](const rl_key_image& x, const rl_key_image& y) {
        return x.limiter != y.limiter ? x.limiter < y.limiter : x.key_hash < y.key_hash;
    });
    return RL_OK;
}

extern "C" int rl_copy_keys(rl_engine* e, size_t n, const uint64_t* key_hash, rl_key_image* out,
                            size_t cap, size_t* n_out) {
    if (!e || n > RL_MOVE_KEYS_MAX || (n && !key_hash) || !n_out || (cap && !out)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    uint32_t count = 0;
    const int rc = move_keys(e, n, key_hash, false, out, cap, &count);
    if (rc != RL_OK) return rc;
    *n_out = count;
    return count > cap ? RL_E_TOO_LARGE : RL_OK;
}

extern "C" int rl_drop_keys(rl_engine* e, size_t n, const uint64_t* key_hash, uint64_t* n_dropped) {
    if (!e || n > RL_MOVE_KEYS_MAX || (n && !key_hash)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    uint32_t count = 0;
    const int rc = move_keys(e, n, key_hash, true, nullptr, 0, &count);
    if (rc == RL_OK && n_dropped) *n_dropped = count;
    return rc;
}

// rl_put_keys with the engine locked and every image's limiter known to exist: the images
// grouped by region on the host, then k_import. *fail = images that found no free slot.
static int put_images_host(rl_engine* e, size_t n, const rl_key_image* in, uint32_t* fail) {
    std::vector<RegionImg> imgs(n);
    for (size_t i = 0; i < n; ++i) {
        RegionImg im = region_img(e, e->lims[in[i].limiter], mix64(in[i].key_hash));
        im.s.a = in[i].word[0]; im.s.b = in[i].word[1]; im.s.c = in[i].word[2];
        im.x = in[i].cache_word;
        imgs[i] = im;
    }
    return apply_region_images(e, imgs, /*with_x=*/true, fail);
}

extern "C" int rl_put_keys(rl_engine* e, size_t n, const rl_key_image* in, size_t* n_put) {
    if (!e || (n && !in)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    for (size_t i = 0; i < n; ++i)
        if (in[i].limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    uint32_t fail = 0;
    const int rc = put_images_host(e, n, in, &fail);
    if (rc != RL_OK) return rc;
    if (n_put) *n_put = n - fail;
    return fail ? RL_E_CAPACITY : RL_OK;
}

// ---------------------------------------------------------------- snapshot / restore
// rl_snapshot_keys(_device), rl_put_keys_device, rl_restore_keys (rl_snapshot.hip; the cut rule
// and ordered form: rl_snapshot.hpp). Like the migration calls they run on the engine stream
// behind every batch submitted before them, work on the table as installed (no collect_status,
// no growth) and touch no batch scratch, d_stats, d_ctl or status word; what the comment above
// says about a put between two batches holds for a whole table of them.
// Device memory, all of it allocated on first use and freed by rl_destroy:
//   e->snap       snap_scratch_bytes() = 8 B per region of a call (kSnapMaxRegions of them) + 48 B
//                 = 512 KiB, whatever the table's size
//   e->put_heads  4 B per image of the largest put so far (the host form: <= max_batch images)
//   e->img_stage  the host forms' images: min(cap, regions of the call x 256) (snapshot) or
//                 min(n, max_batch) (restore) x 48 B, the largest so far
static_assert(RL_SNAPSHOT_MIN_CAP == kSnapRegionSlots && RL_SNAPSHOT_MIN_CAP == kRegionSlots,
              "a cap of one region always makes progress");

static int snap_scratch(rl_engine* e, SnapScratch* sc) {
    const int rc = e->snap.reserve(snap_scratch_bytes());
    if (rc != RL_OK) return rc;
    *sc = snap_scratch_at(e->snap);
    return RL_OK;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The three snapshot launches for limiter `li` on the engine stream; *m_out = regions handled.
static int snapshot_enqueue(rl_engine* e, size_t li, uint64_t region_begin, uint64_t region_count,
                            KeyImage* out, uint64_t cap, uint64_t* hdr, const SnapScratch& sc,
                            uint64_t* m_out) {
    const HostLimiter& h = e->lims[li];
    SnapArgs a{};
    a.L = h.dev;
    a.lim = (uint32_t)li;
    a.regions_total = h.table_bytes / sizeof(Slot) / kRegionSlots;
    a.region_begin = region_begin;
    a.m = (uint32_t)snap_clip(region_begin, region_count, a.regions_total);
    a.cap = std::min<uint64_t>(cap, kSnapMaxImages);
    a.count = sc.count; a.offset = sc.offset; a.out = out; a.hdr = hdr;
    if (m_out) *m_out = a.m;
    HIP_OK(launch_snapshot(a, e->stream));
    return RL_OK;
}

extern "C" int rl_snapshot_keys_device(rl_engine* e, uint16_t limiter, uint64_t region_begin,
                                       uint64_t region_count, rl_key_image* out, size_t cap,
                                       uint64_t* hdr, void* stream) {
    if (!e || !hdr || (cap && !out) || !aligned16(out)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    SnapScratch sc;
    int rc = snap_scratch(e, &sc);
    if (rc != RL_OK) return rc;
    StreamJoin join(e->stream, (hipStream_t)stream);
    HIP_OK(join.err);
    rc = snapshot_enqueue(e, limiter, region_begin, region_count, (KeyImage*)out, cap, hdr, sc, nullptr);
    if (rc != RL_OK) return rc;
    HIP_OK(join.finish());
    return RL_OK;
}

extern "C" int rl_snapshot_keys(rl_engine* e, uint16_t limiter, uint64_t region_begin,
                                uint64_t region_count, rl_key_image* out, size_t cap, size_t* n_out,
                                uint64_t* regions_done, uint64_t* regions_total) {
    if (!e || !n_out || !regions_done || !regions_total || (cap && !out)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    SnapScratch sc;
    int rc = snap_scratch(e, &sc);
    if (rc != RL_OK) return rc;
    const uint64_t total = e->lims[limiter].table_bytes / sizeof(Slot) / kRegionSlots;
    const uint64_t m = snap_clip(region_begin, region_count, total);
    rc = e->img_stage.reserve((size_t)std::min<uint64_t>(cap, m * kRegionSlots));
    if (rc != RL_OK) return rc;
    rc = snapshot_enqueue(e, limiter, region_begin, region_count, e->img_stage, cap, sc.hdr, sc, nullptr);
    if (rc != RL_OK) return rc;
    uint64_t hdr[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(hdr, sc.hdr, sizeof(hdr), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (hdr[0] > cap || hdr[0] > m * kRegionSlots || hdr[1] > m) return RL_E_INTERNAL;
    *regions_total = hdr[2];
    *regions_done = hdr[1];
    if (snap_too_large(m, hdr[1])) {
        *n_out = (size_t)hdr[3];
        return RL_E_TOO_LARGE;
    }
    if (hdr[0]) HIP_OK(hipMemcpy(out, e->img_stage, (size_t)hdr[0] * sizeof(KeyImage), hipMemcpyDeviceToHost));
    *n_out = (size_t)hdr[0];
    return RL_OK;
}

// The ordered put of n device images on the engine stream, its header into `hdr` (device).
static int put_enqueue(rl_engine* e, size_t n, const KeyImage* in, uint64_t* hdr, const SnapScratch& sc) {
    PutArgs a{};
    a.in = in; a.n = (uint32_t)n; a.n_lim = (uint32_t)e->lims.size(); a.shard_bits = e->shard_bits;
    a.lims = e->d_lims; a.heads = e->put_heads; a.ctl = sc.ctl; a.hdr = hdr;
    HIP_OK(launch_put_ordered(a, e->stream));
    return RL_OK;
}

extern "C" int rl_put_keys_device(rl_engine* e, size_t n, const rl_key_image* in, uint64_t* hdr,
                                  void* stream) {
    if (!e || !hdr || (n && !in) || !aligned16(in)) return RL_E_INVALID_ARG;
    if ((uint64_t)n > kSnapMaxImages) return RL_E_TOO_LARGE;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    SnapScratch sc;
    int rc = snap_scratch(e, &sc);
    if (rc == RL_OK) rc = e->put_heads.reserve(n);
    if (rc != RL_OK) return rc;
    StreamJoin join(e->stream, (hipStream_t)stream);
    HIP_OK(join.err);
    rc = put_enqueue(e, n, (const KeyImage*)in, hdr, sc);
    if (rc != RL_OK) return rc;
    HIP_OK(join.finish());
    return RL_OK;
}

extern "C" int rl_restore_keys(rl_engine* e, size_t n, const rl_key_image* in, size_t* n_put) {
    if (!e || (n && !in)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    for (size_t i = 0; i < n; ++i)
        if (in[i].limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    const size_t piece = std::min<size_t>(n, (size_t)std::max<uint64_t>(e->opts.max_batch, 1));
    SnapScratch sc;
    int rc = snap_scratch(e, &sc);
    if (rc == RL_OK) rc = e->put_heads.reserve(piece);
    if (rc == RL_OK) rc = e->img_stage.reserve(piece);
    if (rc != RL_OK) return rc;
    size_t failed = 0;
    for (size_t at = 0; at < n; at += piece) {
        const size_t m = std::min(piece, n - at);
        HIP_OK(hipMemcpyAsync(e->img_stage, in + at, m * sizeof(KeyImage), hipMemcpyHostToDevice, e->stream));
        rc = put_enqueue(e, m, e->img_stage, sc.hdr, sc);
        if (rc != RL_OK) return rc;
        uint64_t hdr[4] = {0, 0, 0, 0};
        HIP_OK(hipMemcpyAsync(hdr, sc.hdr, sizeof(hdr), hipMemcpyDeviceToHost, e->stream));
        HIP_OK(hipStreamSynchronize(e->stream));
        if (hdr[2] & ~(uint64_t)kPutRejectOrder) return RL_E_INTERNAL;   // (limiters were checked)
        if (hdr[2]) {                                 // not in ordered form: nothing was written
            uint32_t f = 0;
            rc = put_images_host(e, m, in + at, &f);
            if (rc != RL_OK) return rc;
            failed += f;
        } else {
            failed += (size_t)hdr[1];
        }
    }
    if (n_put) *n_put = n - failed;
    return failed ? RL_E_CAPACITY : RL_OK;
}

extern "C" int rl_sweep_expired(rl_engine* e, int64_t now_ns, uint64_t* reclaimed) {
    if (!e) return RL_E_INVALID_ARG;
    if (reclaimed) *reclaimed = 0;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    const int64_t now = floor_div_ms(now_ns);
    std::vector<uint32_t> h(e->lims.size() + 1, 0);
    DevArray<uint32_t> d_count;
    if (d_count.reserve(h.size()) != RL_OK) return RL_E_NOMEM;
    HIP_OK(hipMemsetAsync(d_count, 0, h.size() * sizeof(uint32_t), e->stream));
    for (size_t li = 0; li < e->lims.size(); ++li) {
        const HostLimiter& hl = e->lims[li];
        HIP_OK(launch_sweep(hl.dev, hl.table_bytes / sizeof(Slot), now, d_count + li, e->stream));
    }
    HIP_OK(hipMemcpyAsync(h.data(), d_count, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (reclaimed)
        for (uint32_t c : h) *reclaimed += c;
    return RL_OK;
}

// ---------------------------------------------------------------- table shrink
// rl_shrink.hip on the engine stream; the rules in rl_shrink.hpp. The plan reads the table as
// installed, as the census does (no collect_status; no limiter state, batch scratch, d_stats,
// d_ctl or status word is touched). Its scratch (12 B per region + the control block) lives for
// the call only.
static_assert(RL_SHRINK_FILL_MAX == kShrinkFillMax && RL_SHRINK_LEVELS == kShrinkLevels, "shrink constants");
static_assert(2 * RL_SHRINK_FILL_MAX == kGrowUsed, "a shrunk region doubles its keys before it flags growth");
static_assert(sizeof(rl_shrink_report) == 8 * 5 + 4 * RL_SHRINK_LEVELS, "rl_shrink_report layout");

// (e->mu held) The plan of limiter li at now_ms into *rep; synchronises e->stream.
static int shrink_plan_locked(rl_engine* e, size_t li, int64_t now_ms, uint64_t min_keys,
                              rl_shrink_report* rep) {
    const HostLimiter& h = e->lims[li];
    const int k = h.dev.region_bits;
    const uint64_t n_regions = 1ULL << k;
    const uint32_t levels = shrink_levels(k);
    DevArray<unsigned char> buf;
    if (buf.reserve(shrink_scratch_bytes(n_regions)) != RL_OK) return RL_E_NOMEM;
    const ShrinkScratch sc = shrink_scratch_at(buf, n_regions);
    ShrinkCtl c;
    HIP_OK(launch_shrink_plan(sc, h.dev, n_regions, levels, now_ms, e->stream));
    HIP_OK(hipMemcpyAsync(&c, sc.ctl, sizeof(c), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    rl_shrink_report r{};
    r.slots_before = h.table_bytes / sizeof(Slot);
    r.used_before = c.used;
    r.kept = c.kept;
    r.levels = levels;
    for (uint32_t i = 0; i < levels; ++i) r.fullest[i] = c.fullest[i];
    r.halvings = shrink_halvings(r.fullest, levels, r.slots_before, min_keys, e->opts.shard_count);
    r.slots_after = r.slots_before >> r.halvings;
    *rep = r;
    return RL_OK;
}

extern "C" int rl_shrink_plan(rl_engine* e, uint16_t limiter, int64_t now_ns, uint64_t min_keys,
                              rl_shrink_report* out) {
    if (!e || !out) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    rl_shrink_report r;
    const int rc = shrink_plan_locked(e, limiter, floor_div_ms(now_ns), min_keys, &r);
    if (rc == RL_OK) *out = r;
    return rc;
}

// Halve limiter li's region count j times: ceil(j / 3) merge passes (k_shrink_merge) through
// fresh tables, the keep rule of the sweep in the first one; the old table is freed and the
// limiter record changed only after the last pass has succeeded and placed every slot. Then,
// as grow_once: region ids of the later limiters shifted, the route lists cleared.
static int shrink_by(rl_engine* e, size_t li, uint32_t j, int64_t now_ms) {
    HostLimiter& h = e->lims[li];
    DevLimiter& d = h.dev;
    const int k = d.region_bits;
    if (j == 0 || (int)j > k - kBinShift) return RL_E_INTERNAL;
    struct Tab { void* t = nullptr; void* x = nullptr; };
    std::vector<Tab> tabs(shrink_passes(j));
    DevArray<uint32_t> fail;
    auto drop = [&] { for (Tab& t : tabs) { dfree(t.t); dfree(t.x); } };
    int rc = fail.reserve(1);
    int bits = k;
    for (uint32_t p = 0; p < tabs.size() && rc == RL_OK; ++p) {
        bits -= (int)shrink_pass_bits(j, p);
        const size_t slots = (size_t)(1ULL << bits) * kRegionSlots;
        rc = dalloc(&tabs[p].t, slots * sizeof(Slot));
        if (rc == RL_OK && h.cache_table) rc = dalloc(&tabs[p].x, slots * sizeof(uint64_t));
    }
    if (rc != RL_OK) { drop(); return rc; }
    hipError_t he = hipMemsetAsync(fail, 0, sizeof(uint32_t), e->stream);
    const void* src_t = h.table;
    const void* src_x = h.cache_table;
    bits = k;
    for (uint32_t p = 0; p < tabs.size() && he == hipSuccess; ++p) {
        const uint32_t s = shrink_pass_bits(j, p);
        bits -= (int)s;
        he = launch_shrink_merge((const Slot*)src_t, (const uint64_t*)src_x, (Slot*)tabs[p].t,
                                 (uint64_t*)tabs[p].x, 1ULL << bits, s, d, now_ms, p == 0, fail, e->stream);
        src_t = tabs[p].t;
        src_x = tabs[p].x;
    }
    uint32_t failed = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&failed, fail, sizeof(failed), hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess) {
        std::fprintf(stderr, "rl_engine: table shrink failed: %s\n", hipGetErrorString(he));
        (void)hipStreamSynchronize(e->stream);       // nothing may still write the tables freed here
        drop();
        return RL_E_DEVICE;
    }
    if (failed) { drop(); return RL_E_INTERNAL; }    // (the plan excludes it; the old table stands)
    Tab last = tabs.back();
    tabs.pop_back();
    drop();                                          // the intermediate tables
    dfree(h.table); dfree(h.cache_table);
    h.table = last.t; h.cache_table = last.x;
    h.table_bytes = (size_t)(1ULL << bits) * kRegionSlots * sizeof(Slot);
    d.table = (uint64_t)(uintptr_t)last.t;
    d.cache_table = (uint64_t)(uintptr_t)last.x;
    d.region_bits = bits;
    uint32_t base = 0;
    for (auto& l : e->lims) { l.dev.region_base = base; base += 1u << l.dev.region_bits; }
    e->n_regions = base;
    // region ids changed: the next batch routes nothing (its hot preparation lists anew)
    HIP_OK(hipMemset(e->route_list, 0xFF, 2 * kRouteWords * sizeof(uint32_t)));
    return upload_limiters(e);
}

extern "C" int rl_shrink_limiter(rl_engine* e, uint16_t limiter, int64_t now_ns, uint64_t min_keys,
                                 rl_shrink_report* out) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);           // held across plan and merge: the plan's proof stands
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    HIP_OK(hipStreamSynchronize(e->stream));         // nothing in flight, as for grow_once
    if (e->pstream) HIP_OK(hipStreamSynchronize(e->pstream));
    const int64_t now = floor_div_ms(now_ns);
    rl_shrink_report r;
    int rc = shrink_plan_locked(e, limiter, now, min_keys, &r);
    if (rc != RL_OK) return rc;
    if (r.halvings) rc = shrink_by(e, limiter, r.halvings, now);
    if (rc == RL_OK && out) *out = r;
    return rc;
}
