// rl_engine.cpp — host runtime behind include/rl_engine.h.
//
// Owns, per GPU: the HBM state table (one region array per limiter), the
// limiter table, the batch scratch and one HIP stream. A batch is a fixed chain
// of kernel launches on that stream (see csrc/rl_*.hip); nothing in the chain
// synchronises with the host, so the device entry point is fully asynchronous.
//
// This unit: create and destroy, limiters and their growth, rl_tune, rl_sync, statistics and
// stage times, rl_debug_fetch, pinned host buffers. Batches: rl_engine_batch.cpp; queries:
// rl_engine_query.cpp; routing: rl_engine_route.cpp; table state: rl_engine_state.cpp.
#include <atomic>
#include <cmath>
#include <new>

#include "rl_engine_impl.hpp"
#include "rl_keys.hpp"

using namespace rl;

namespace {
constexpr int kStages = 11;
// (two-pass batches: "group" is k_group; "scan1" / "scatter1" are empty since round 6, when
// k_group replaced the global second pass)
const char* kStageNames[kStages] = {"upsweep0", "scan0", "scatter0", "group", "scan1",
                                    "scatter1", "region_offsets", "region", "unpermute", "total",
                                    "hot_fill"};
const int kStagePairs[kStages][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 6},
                                     {6, 7}, {7, 8}, {8, 9}, {0, 9}, {10, 11}};
}  // namespace

static void ensure_events(rl_engine* e) {
    if (e->ev[0][0]) return;
    for (int r = 0; r < kEvRing; ++r)
        for (int i = 0; i < kMarks; ++i) (void)hipEventCreate(&e->ev[r][i]);
}

// rl_debug_alloc_fill: -1 off, else the byte every new device allocation is filled with.
static std::atomic<int> g_alloc_fill{-1};

namespace rl {
hipError_t dev_malloc(void** p, size_t bytes) {
    hipError_t he = hipMalloc(p, bytes);
    const int fill = g_alloc_fill.load(std::memory_order_relaxed);
    if (he == hipSuccess && fill >= 0) {
        he = hipMemset(*p, fill, bytes);           // (synchronous: done before any later use)
        if (he == hipSuccess) he = hipDeviceSynchronize();
        if (he != hipSuccess) { (void)hipFree(*p); *p = nullptr; }
    }
    return he;
}
}  // namespace rl

extern "C" int rl_debug_alloc_fill(int byte) {
    if (byte < -1 || byte > 255) return RL_E_INVALID_ARG;
    g_alloc_fill.store(byte, std::memory_order_relaxed);
    return RL_OK;
}

extern "C" int rl_abi_version(void) { return RL_ABI_VERSION; }

extern "C" const char* rl_strerror(int s) {
    switch (s) {
        case RL_OK: return "ok";
        case RL_E_INVALID_ARG: return "invalid argument";
        case RL_E_INVALID_REQUEST: return "invalid request(s) in batch (permits <= 0 or unknown limiter)";
        case RL_E_CAPACITY: return "state-table region full";
        case RL_E_DEVICE: return "HIP device error";
        case RL_E_NOMEM: return "out of memory";
        case RL_E_TOO_LARGE: return "batch larger than max_batch";
        case RL_E_LIMITERS: return "too many limiters";
        case RL_E_INTERNAL: return "internal error (engine logic)";
        default: return "unknown status";
    }
}

extern "C" uint32_t rl_owner_of(uint64_t key_hash, uint16_t, uint32_t shard_count) {
    if (shard_count <= 1) return 0;
    const int s = ceil_log2(shard_count);
    return (uint32_t)(mix64(key_hash) >> (64 - s));
}

extern "C" int rl_create(const rl_opts* opts, rl_engine** out) {
    if (!out) return RL_E_INVALID_ARG;
    *out = nullptr;
    rl_opts o{};
    if (opts) o = *opts;
    if (o.max_batch == 0) o.max_batch = 1u << 22;
    if (o.max_batch > 0xFFFFFFF0ULL) return RL_E_INVALID_ARG;   // u32 positions
    if (o.default_capacity == 0) o.default_capacity = 1u << 20;
    if (o.shard_count == 0) o.shard_count = 1;
    if ((o.shard_count & (o.shard_count - 1)) != 0 || o.shard_count > 64) return RL_E_INVALID_ARG;
    if (o.shard_index >= o.shard_count) return RL_E_INVALID_ARG;
    if (o.max_skew_ms < 0) return RL_E_INVALID_ARG;
    rl_engine* e = new (std::nothrow) rl_engine();
    if (!e) return RL_E_NOMEM;
    e->opts = o;
    e->shard_bits = ceil_log2(o.shard_count);
    if (o.device >= 0) {
        if (hipSetDevice(o.device) != hipSuccess) { delete e; return RL_E_DEVICE; }
        e->device = o.device;
    } else {
        (void)hipGetDevice(&e->device);
    }
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
        rl_destroy(e);
        return RL_E_DEVICE;
    }
    // The hot chains' stream has the device's highest priority: their workgroups are a few
    // long sequential critical paths launched beside ~10^5-10^6 short normal-region waves,
    // and at equal priority the dispatcher interleaved the two launches, so some chains
    // only started once normal regions had drained (sw_zipf: up to 2.5 ms late).
    int prio_least = 0, prio_greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_greatest = 0;
    if (hipStreamCreateWithPriority(&e->hstream, hipStreamNonBlocking, prio_greatest) != hipSuccess ||
        hipEventCreateWithFlags(&e->hot_ev[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->hot_ev[1], hipEventDisableTiming) != hipSuccess) {
        rl_destroy(e);
        return RL_E_DEVICE;
    }
    e->timing = (o.flags & RL_OPT_STAGE_TIMING) != 0;
    if (e->timing) ensure_events(e);
    e->pipeline = (o.flags & RL_OPT_PIPELINE) != 0;
    e->auto_grow = (o.flags & RL_OPT_FIXED_CAPACITY) == 0;
    if (e->pipeline && hipStreamCreateWithFlags(&e->pstream, hipStreamNonBlocking) != hipSuccess) {
        rl_destroy(e);
        return RL_E_DEVICE;
    }
    int rc = RL_OK;
    if (e->pipeline && hipEventCreateWithFlags(&e->in_ev, hipEventDisableTiming) != hipSuccess)
        rc = RL_E_DEVICE;
    for (int k = 0; k < (e->pipeline ? 2 : 1); ++k) {
        BatchScratch& B = e->sc[k];
        if (rc == RL_OK) rc = B.d_ctl.reserve(1);
        if (rc == RL_OK) rc = B.bin_total.reserve(1u << kMaxDigitBits);
        if (rc == RL_OK) rc = B.bin_base.reserve(1u << kMaxDigitBits);
        // a batch writes its nb0 pass-0 bins only; rl_debug_fetch("bin_totals") copies all of them
        if (rc == RL_OK && (hipMemset(B.bin_total, 0, sizeof(uint32_t) << kMaxDigitBits) != hipSuccess ||
                            hipMemset(B.bin_base, 0, sizeof(uint32_t) << kMaxDigitBits) != hipSuccess))
            rc = RL_E_DEVICE;
        if (rc == RL_OK && e->pipeline &&
            (hipEventCreateWithFlags(&B.parted, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&B.freed, hipEventDisableTiming) != hipSuccess))
            rc = RL_E_DEVICE;
    }
    if (rc == RL_OK) rc = e->d_stats.reserve((size_t)kStatSlots * kStWords);
    if (rc == RL_OK && hipMemset(e->d_stats, 0, (size_t)kStatSlots * kStWords * 8) != hipSuccess)
        rc = RL_E_DEVICE;
    if (rc == RL_OK && hipHostMalloc((void**)&e->h_ctl, sizeof(BatchCtl)) != hipSuccess) rc = RL_E_NOMEM;
    if (rc == RL_OK) rc = e->d_lims.reserve(RL_MAX_LIMITERS);
    if (rc == RL_OK) rc = e->hot_list.reserve(kHotListWords);
    if (rc == RL_OK) rc = e->hot_info.reserve(kHotMax);
    if (rc == RL_OK) rc = e->route_list.reserve(2 * kRouteWords);
    if (rc == RL_OK) rc = e->route_start.reserve(2 * kRouteSlots);
    if (rc == RL_OK) rc = e->route_cnt.reserve(2 * kRouteSlots);
    if (rc == RL_OK) rc = e->order_meta.reserve(kOrderMeta);
    if (rc == RL_OK) rc = e->solo_list.reserve(kSoloMax + 1);
    if (rc == RL_OK && hipMemset(e->route_list, 0xFF, 2 * kRouteWords * sizeof(uint32_t)) != hipSuccess)
        rc = RL_E_DEVICE;
    if (rc != RL_OK) { rl_destroy(e); return rc; }
    std::memset(e->h_ctl, 0, sizeof(BatchCtl));
    *out = e;
    return RL_OK;
}

extern "C" void rl_destroy(rl_engine* e) {
    if (!e) return;
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->pstream) (void)hipStreamSynchronize(e->pstream);
    if (e->hstream) (void)hipStreamSynchronize(e->hstream);
    for (auto& l : e->lims) { dfree(l.table); dfree(l.cache_table); }
    for (auto& pb : e->pinned) (void)hipHostUnregister(pb.first);
    if (e->h_ctl) (void)hipHostFree(e->h_ctl);
    if (e->sm_block) (void)hipHostFree(e->sm_block);
    for (BatchScratch& B : e->sc) {
        if (B.parted) (void)hipEventDestroy(B.parted);
        if (B.freed) (void)hipEventDestroy(B.freed);
    }
    for (int r = 0; r < kEvRing; ++r)
        for (int i = 0; i < kMarks; ++i) if (e->ev[r][i]) (void)hipEventDestroy(e->ev[r][i]);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    if (e->pstream) (void)hipStreamDestroy(e->pstream);
    if (e->in_ev) (void)hipEventDestroy(e->in_ev);
    if (e->hstream) (void)hipStreamDestroy(e->hstream);
    for (hipEvent_t ev : e->hot_ev) if (ev) (void)hipEventDestroy(ev);
    delete e;
}

int upload_limiters(rl_engine* e) {
    std::vector<DevLimiter> dv;
    for (auto& l : e->lims) dv.push_back(l.dev);
    HIP_OK(hipMemcpy(e->d_lims, dv.data(), dv.size() * sizeof(DevLimiter), hipMemcpyHostToDevice));
    std::vector<uint8_t> map(e->n_regions);
    for (size_t li = 0; li < e->lims.size(); ++li) {
        const auto& d = e->lims[li].dev;
        std::fill(map.begin() + d.region_base, map.begin() + d.region_base + (1u << d.region_bits),
                  (uint8_t)li);
    }
    if (e->d_region_lim.reserve(map.size()) != RL_OK) return RL_E_NOMEM;
    HIP_OK(hipMemcpy(e->d_region_lim, map.data(), map.size(), hipMemcpyHostToDevice));
    return RL_OK;
}

// kLfPctMul / kLfPctFma (rl_device.hpp): checked for every remainder of windows up to 2^22 ms.
static uint32_t pct_flags(int64_t w, double inv) {
    if (w > (int64_t(1) << 22)) return 0;
    const double dw = (double)w;
    bool mul = true, fma = true;
    for (int64_t r = 1; r < w && (mul || fma); ++r) {
        const double dr = (double)r, exact = dr / dw, q = dr * inv;
        if (q != exact) mul = false;
        if (std::fma(std::fma(-q, dw, dr), inv, q) != exact) fma = false;
    }
    return mul ? kLfPctMul : fma ? kLfPctFma : 0u;
}

extern "C" int rl_add_limiter_ex(rl_engine* e, const rl_limiter_config* c, uint16_t* id) {
    if (!e || !c) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    // RateLimitConfig.validate() (RateLimitConfig.java:46-56)
    if (c->max_permits <= 0 || c->window_ms <= 0 || !(c->refill_per_s >= 0.0)) return RL_E_INVALID_ARG;
    if ((c->flags & ~RL_LIM_LOCAL_CACHE) != 0 || c->local_cache_ttl_ms < 0) return RL_E_INVALID_ARG;
    if (c->algo == RL_ALGO_TOKEN_BUCKET && !(c->refill_per_s > 0.0)) return RL_E_INVALID_ARG;  // TB ctor :77-79
    if (c->algo != RL_ALGO_TOKEN_BUCKET && c->algo != RL_ALGO_SLIDING_WINDOW) return RL_E_INVALID_ARG;
    if (c->window_ms > RL_MAX_WINDOW_MS) return RL_E_INVALID_ARG;
    if (c->algo == RL_ALGO_SLIDING_WINDOW && c->max_permits > RL_SW_MAX_PERMITS_LIMIT) return RL_E_INVALID_ARG;
    if (c->algo == RL_ALGO_TOKEN_BUCKET && c->max_permits > RL_TB_MAX_PERMITS_LIMIT) return RL_E_INVALID_ARG;
    if (e->lims.size() >= RL_MAX_LIMITERS) return RL_E_LIMITERS;
    (void)hipSetDevice(e->device);
    HostLimiter h;
    h.cfg = *c;
    uint64_t cap = c->capacity ? c->capacity : e->opts.default_capacity;
    uint64_t per_shard = (cap + e->opts.shard_count - 1) / e->opts.shard_count;
    uint64_t slots = std::max<uint64_t>(per_shard * 2, kRegionSlots);   // load <= 0.5
    uint64_t regions = (slots + kRegionSlots - 1) / kRegionSlots;
    int k = std::max(ceil_log2(regions), kBinShift);     // whole bins of kRegionsPerBin regions
    if (k + e->shard_bits > 40) return RL_E_INVALID_ARG;
    if ((uint64_t)e->n_regions + (1ULL << k) > (1ULL << 24)) return RL_E_LIMITERS;
    DevLimiter& d = h.dev;
    std::memset(&d, 0, sizeof(d));
    d.algo = c->algo;
    d.region_bits = k;
    d.region_base = e->n_regions;
    d.max_permits = c->max_permits;
    d.window_ms = c->window_ms;
    d.ttl_ms = c->algo == RL_ALGO_TOKEN_BUCKET ? c->window_ms * 2 : c->window_ms;
    d.rate_per_ms = c->refill_per_s / 1000.0;        // TokenBucketRateLimiter.java:85
    d.inv_rate = d.rate_per_ms > 0.0 ? 1.0 / d.rate_per_ms : 0.0;
    d.inv_window = 1.0 / (double)c->window_ms;
    d.lflags = pct_flags(c->window_ms, d.inv_window);
    d.capacity = (double)c->max_permits;
    h.table_bytes = (size_t)(1ULL << k) * kRegionSlots * sizeof(Slot);
    if (dalloc(&h.table, h.table_bytes) != RL_OK) return RL_E_NOMEM;
    if (hipMemset(h.table, 0, h.table_bytes) != hipSuccess) { dfree(h.table); return RL_E_DEVICE; }
    d.table = (uint64_t)(uintptr_t)h.table;
    if (c->algo == RL_ALGO_SLIDING_WINDOW && (c->flags & RL_LIM_LOCAL_CACHE) && c->local_cache_ttl_ms > 0) {
        const size_t xb = (size_t)(1ULL << k) * kRegionSlots * sizeof(uint64_t);
        if (dalloc(&h.cache_table, xb) != RL_OK) { dfree(h.table); return RL_E_NOMEM; }
        if (hipMemset(h.cache_table, 0, xb) != hipSuccess) { dfree(h.table); dfree(h.cache_table); return RL_E_DEVICE; }
        d.cache_table = (uint64_t)(uintptr_t)h.cache_table;
        d.cache_ttl_ms = c->local_cache_ttl_ms;
    }
    e->lims.push_back(h);
    e->n_regions += 1u << k;
    int rc = upload_limiters(e);
    if (rc != RL_OK) return rc;
    if (id) *id = (uint16_t)(e->lims.size() - 1);
    return RL_OK;
}

extern "C" int rl_add_limiter(rl_engine* e, int algo, int64_t max_permits, int64_t window_ms,
                              double refill_per_s, uint16_t* id) {
    rl_limiter_config c{};
    c.algo = algo;
    c.max_permits = max_permits;
    c.window_ms = window_ms;
    c.refill_per_s = refill_per_s;
    c.capacity = 0;                                  // local cache off: the parity-mode default
    return rl_add_limiter_ex(e, &c, id);
}

// Double limiter li's region count (k -> k + 1 region bits): new table, every old region
// split in two by k_grow, old table freed, region ids of the later limiters shifted.
// Synchronous; nothing may be in flight on the engine's streams.
int grow_once(rl_engine* e, size_t li) {
    HostLimiter& h = e->lims[li];
    DevLimiter& d = h.dev;
    const int k = d.region_bits;
    if (k + 1 + e->shard_bits > 40 || (uint64_t)e->n_regions + (1ULL << k) > (1ULL << 24))
        return RL_E_LIMITERS;
    HIP_OK(hipStreamSynchronize(e->stream));
    if (e->pstream) HIP_OK(hipStreamSynchronize(e->pstream));
    const size_t nb = h.table_bytes * 2;
    void* nt = nullptr;
    void* nx = nullptr;
    if (dalloc(&nt, nb) != RL_OK) return RL_E_NOMEM;
    if (h.cache_table && dalloc(&nx, nb / sizeof(Slot) * sizeof(uint64_t)) != RL_OK) {
        dfree(nt);
        return RL_E_NOMEM;
    }
    if (launch_grow((const Slot*)h.table, (const uint64_t*)h.cache_table, (Slot*)nt, (uint64_t*)nx,
                    1ULL << k, e->shard_bits, k + 1, d.algo, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess) {
        dfree(nt); dfree(nx);
        return RL_E_DEVICE;
    }
    dfree(h.table); dfree(h.cache_table);
    h.table = nt; h.cache_table = nx; h.table_bytes = nb;
    d.table = (uint64_t)(uintptr_t)nt;
    d.cache_table = (uint64_t)(uintptr_t)nx;
    d.region_bits = k + 1;
    uint32_t base = 0;
    for (auto& l : e->lims) { l.dev.region_base = base; base += 1u << l.dev.region_bits; }
    e->n_regions = base;
    ++e->grows;
    // region ids changed: the next batch routes nothing (its hot preparation lists anew)
    HIP_OK(hipMemset(e->route_list, 0xFF, 2 * kRouteWords * sizeof(uint32_t)));
    return upload_limiters(e);
}

static int grow_to(rl_engine* e, size_t li, uint64_t min_keys) {
    const uint64_t per_shard = (min_keys + e->opts.shard_count - 1) / e->opts.shard_count;
    while ((e->lims[li].table_bytes / sizeof(Slot)) < per_shard * 2) {   // load <= 0.5
        const int rc = grow_once(e, li);
        if (rc != RL_OK) return rc;
    }
    return RL_OK;
}

extern "C" int rl_grow_limiter(rl_engine* e, uint16_t limiter, uint64_t min_keys) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    return grow_to(e, limiter, min_keys);
}

extern "C" int rl_limiter_slots(rl_engine* e, uint16_t limiter, uint64_t* slots) {
    if (!e || !slots) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    *slots = e->lims[limiter].table_bytes / sizeof(Slot);
    return RL_OK;
}

// Page-lock a caller's host buffer so the host-buffer entry points DMA it directly instead
// of staging it through the runtime's bounce buffers (pageable memory). Registering an
// already page-locked range (hipHostMalloc, another registration) is a no-op.
extern "C" int rl_pin_host(rl_engine* e, void* ptr, size_t bytes) {
    if (!e || !ptr || bytes == 0) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    for (auto& pb : e->pinned)
        if (pb.first == ptr) return pb.second >= bytes ? RL_OK : RL_E_INVALID_ARG;
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, ptr) == hipSuccess && at.type == hipMemoryTypeHost) {
        (void)hipGetLastError();
        return RL_OK;                               // already page-locked by its owner
    }
    (void)hipGetLastError();
    if (hipHostRegister(ptr, bytes, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return RL_E_DEVICE;
    }
    e->pinned.emplace_back(ptr, bytes);
    return RL_OK;
}

// Undo rl_pin_host; must be called before the caller frees the buffer. Unknown pointers
// (never pinned by this engine) return RL_E_INVALID_ARG.
extern "C" int rl_unpin_host(rl_engine* e, void* ptr) {
    if (!e || !ptr) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    for (size_t i = 0; i < e->pinned.size(); ++i) {
        if (e->pinned[i].first != ptr) continue;
        (void)hipStreamSynchronize(e->stream);     // no copy of it in flight
        const hipError_t r = hipHostUnregister(ptr);
        e->pinned.erase(e->pinned.begin() + (long)i);
        return r == hipSuccess ? RL_OK : RL_E_DEVICE;
    }
    return RL_E_INVALID_ARG;
}

extern "C" int rl_batch_stats_get(rl_engine* e, rl_batch_stats* out) {
    if (!e || !out) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    collect_status(e);
    const BatchCtl& c = *e->h_ctl;
    out->n = e->last_n;
    out->allowed = c.allowed;
    out->distinct_keys = c.distinct;
    out->invalid = c.invalid;
    out->capacity_errors = c.cap_err;
    out->regions_touched = c.regions;
    out->table_bytes = c.table_bytes;
    out->cache_hits = c.cache_hits;
    out->table_grows = e->grows;
    out->hot_regions = c.n_hot;
    out->routed = e->last_n >= c.n_normal ? e->last_n - c.n_normal : 0;
    return RL_OK;
}

// Average per-stage milliseconds over the batches enqueued since the previous call
// (at most the last 64). Stages a batch did not run (second pass) read 0.
extern "C" int rl_stage_times(rl_engine* e, const char** names, float* ms, int cap) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    collect_status(e);
    const int k = std::min(cap, kStages);
    const int nb = e->ring_used;
    for (int i = 0; i < k; ++i) {
        double acc = 0.0;
        for (int b = 0; b < nb; ++b) {
            const int r = (e->ring_next - 1 - b + kEvRing) % kEvRing;
            float x = 0.f;
            if (hipEventElapsedTime(&x, e->ev[r][kStagePairs[i][0]], e->ev[r][kStagePairs[i][1]]) != hipSuccess)
                x = 0.f;
            acc += x;
        }
        if (names) names[i] = kStageNames[i];
        if (ms) ms[i] = (e->timing && nb) ? (float)(acc / nb) : -1.f;
    }
    e->ring_used = 0;
    return k;
}

extern "C" int rl_tune(rl_engine* e, const char* key, int64_t value) {
    if (!e || !key) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
#if RL_MEASURE   // (rl_launch.hpp) a key of the measurement build only
    if (std::strcmp(key, "ablate") == 0) { e->ablate = (uint32_t)value; return RL_OK; }
#endif
    if (std::strcmp(key, "upsweep_per_cu") == 0) { e->tune.up_per_cu = (uint32_t)value; return RL_OK; }
    if (std::strcmp(key, "scatter_per_cu") == 0) { e->sc_per_cu = (uint32_t)value; return RL_OK; }
    if (std::strcmp(key, "scatter_split") == 0) { e->sc_split = value != 0; return RL_OK; }
    if (std::strcmp(key, "unpermute_split") == 0) { e->un_split = (uint32_t)value; return RL_OK; }
    if (std::strcmp(key, "mid_xcd") == 0) { e->mid_xcd = value ? 1u : 0u; return RL_OK; }
    if (std::strcmp(key, "unpermute_per_cu") == 0) { e->un_per_cu = (uint32_t)value; return RL_OK; }
    if (std::strcmp(key, "digest_per_cu") == 0) {      // k_digest workgroups per CU; 0 = default
        if (value < 0 || value > 64) return RL_E_INVALID_ARG;
        e->digest_per_cu = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "key_stage_bytes") == 0) {    // blob stage of the string-key host forms
        if (value < (int64_t)kKeyMaxBytes || value > ((int64_t)1 << 32)) return RL_E_INVALID_ARG;
        e->key_stage_bytes = (size_t)value;            // (allocated by the next call that stages)
        return RL_OK;
    }
    if (std::strcmp(key, "keys_direct") == 0) { e->keys_direct = value != 0; return RL_OK; }
    if (std::strcmp(key, "debug_regions") == 0) { e->debug_regions = value != 0; return RL_OK; }
    if (std::strcmp(key, "wide_records") == 0) { e->force_wide = value != 0; return RL_OK; }
    if (std::strcmp(key, "stage_timing") == 0) {     // hipEvents around every stage on/off
        if (value) ensure_events(e);
        e->timing = value != 0;
        e->ring_used = 0;
        return RL_OK;
    }
    if (std::strcmp(key, "hot_threshold") == 0) {      // records per region; 0 = no hot path
        if (value < 0 || value > 0xFFFFFFFFLL) return RL_E_INVALID_ARG;
        e->tune.hot_threshold = (uint32_t)value;
        e->tune.hot_thr_auto = false;
        return RL_OK;
    }
    if (std::strcmp(key, "solo_threshold") == 0) {     // records per region; 0 = off
        if (value < 0 || value > 0xFFFFFFFFLL) return RL_E_INVALID_ARG;
        e->solo_threshold = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "sparse_max") == 0) {         // records per region; 0 = image mode only
        if (value < 0 || value > 0xFFFFFFFFLL) return RL_E_INVALID_ARG;
        e->sparse_max = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "region_order") == 0) {
        e->region_order = value != 0;
        return RL_OK;
    }
    if (std::strcmp(key, "order_prefix") == 0) {
        if (value < 0) return RL_E_INVALID_ARG;
        e->order_prefix = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "route") == 0) {             // hot-region routing in pass 0
        e->tune.route = value != 0;
        return RL_OK;
    }
    if (std::strcmp(key, "tile_items") == 0) {        // partition tile = value x 512 requests
        if (value != 0 && (value < 8 || value > 1024 || value % 8 != 0)) return RL_E_INVALID_ARG;
        e->tune.tile_items = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "segments") == 0) {          // two-pass batches: pass-0 output segments
        if (value < 1 || value > 64) return RL_E_INVALID_ARG;
        e->tune.segments = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "group_bits") == 0) {        // two-pass batches: pass-0 high-digit bits
        if (value < 1 || value > kMaxDigitBits) return RL_E_INVALID_ARG;
        e->tune.group_bits = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "walk") == 0) {              // allow walks of the hot chains
        e->walk = value != 0;
        if (!e->walk && e->walk_tab) {                 // (hipFree waits for the batches in flight)
            HIP_OK(hipStreamSynchronize(e->stream));
            if (e->hstream) HIP_OK(hipStreamSynchronize(e->hstream));
            e->walk_tab.free();
        }
        return RL_OK;
    }
    if (std::strcmp(key, "chain_split") == 0) {       // a hot region's other keys on a second wave
        e->chain_split = value != 0;
        return RL_OK;
    }
    if (std::strcmp(key, "walk_min") == 0) {          // keys walked: at least this many allows expected
        if (value < 0 || value > 0xFFFFFFFFLL) return RL_E_INVALID_ARG;
        e->walk_min = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "hot_epoch") == 0) {         // the hot marks' epoch as is (tests of its wrap)
        e->epoch = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "small_batch") == 0) {       // batches up to `value` requests ask for the small path; 0 = off
        if (value < 0) return RL_E_INVALID_ARG;
        e->small_batch = (uint64_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "fail_batches") == 0) {      // the next `value` batches fail (RL_E_DEVICE)
        if (value < 0 || value > 0xFFFFFFFFLL) return RL_E_INVALID_ARG;
        e->inject_fail = (uint32_t)value;
        return RL_OK;
    }
    return RL_E_INVALID_ARG;
}

extern "C" int rl_sync(rl_engine* e) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_OK(hipStreamSynchronize(e->stream));
    if (e->pstream) HIP_OK(hipStreamSynchronize(e->pstream));
    if (e->pending_status && !e->last_small) {               // the last batch is complete
        e->hot_hint = e->h_ctl->n_hot;
        e->walk_hint = e->h_ctl->n_walk;
    }
    return RL_OK;
}

extern "C" int rl_debug_fetch(rl_engine* e, const char* what, void* out, size_t bytes) {
    if (!e || !what || (!out && bytes)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (std::strcmp(what, "region_times") == 0) {
        if (!e->dbg) return RL_E_INVALID_ARG;
        HIP_OK(hipStreamSynchronize(e->stream));
        const size_t nb = std::min(bytes, e->dbg.cap * sizeof(uint64_t));
        HIP_OK(hipMemcpy(out, e->dbg, nb, hipMemcpyDeviceToHost));
        return (int)(nb / (kDbgWords * sizeof(uint64_t)));
    }
    if (std::strcmp(what, "bin_totals") == 0) {      // the last batch's pass-0 bin sizes
        const BatchScratch& B = e->sc[e->pipeline ? e->next_set ^ 1 : 0];
        HIP_OK(hipStreamSynchronize(e->stream));
        const size_t nb = std::min(bytes, ((size_t)1 << kMaxDigitBits) * sizeof(uint32_t));
        HIP_OK(hipMemcpy(out, B.bin_total, nb, hipMemcpyDeviceToHost));
        return (int)(nb / sizeof(uint32_t));
    }
    if (std::strcmp(what, "alloc_probe") == 0) {     // a fresh allocation as dev_malloc hands it out
        if (bytes == 0 || bytes > ((size_t)1 << 20)) return RL_E_INVALID_ARG;
        DevArray<uint8_t> probe;
        if (probe.reserve(bytes) != RL_OK) return RL_E_NOMEM;
        HIP_OK(hipMemcpy(out, probe, bytes, hipMemcpyDeviceToHost));
        return (int)bytes;
    }
    if (std::strcmp(what, "usage_passes") == 0) {    // table passes of the last rl_top_consumers
        if (bytes < sizeof(uint32_t)) return RL_E_INVALID_ARG;
        std::memcpy(out, &e->usage_passes, sizeof(uint32_t));
        return 1;
    }
#ifdef RL_RETRY_COUNT
    if (std::strcmp(what, "retry_counts") == 0) {    // {searches, bisections, buckets probed}
        if (!e->retry_dbg || bytes < 3 * sizeof(unsigned long long)) return RL_E_INVALID_ARG;   // since the last fetch
        HIP_OK(hipStreamSynchronize(e->stream));
        HIP_OK(hipMemcpy(out, e->retry_dbg, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIP_OK(hipMemset(e->retry_dbg, 0, 3 * sizeof(unsigned long long)));
        return 3;
    }
#endif
    return RL_E_INVALID_ARG;
}
