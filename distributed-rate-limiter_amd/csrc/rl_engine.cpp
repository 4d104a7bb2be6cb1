// rl_engine.cpp — host runtime behind include/rl_engine.h.
//
// Owns, per GPU: the HBM state table (one region array per limiter), the
// limiter table, the batch scratch and one HIP stream. A batch is a fixed chain
// of kernel launches on that stream (see csrc/rl_*.hip); nothing in the chain
// synchronises with the host, so the device entry point is fully asynchronous.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "../../include/rl_engine.h"
#include "rl_keys.hpp"
#include "rl_launch.hpp"
#include "rl_shrink.hpp"
#include "rl_snapshot.hpp"

using namespace rl;

namespace {

// Stage timing: events bracket every kernel of a batch; a ring of per-batch event
// sets is averaged when rl_stage_times is called (no host sync inside a batch).
constexpr int kMarks = 12;   // marks 0..11 on the engine stream
constexpr int kStages = 11;
// (two-pass batches: "group" is k_group; "scan1" / "scatter1" are empty since round 6, when
// k_group replaced the global second pass)
const char* kStageNames[kStages] = {"upsweep0", "scan0", "scatter0", "group", "scan1",
                                    "scatter1", "region_offsets", "region", "unpermute", "total",
                                    "hot_fill"};
const int kStagePairs[kStages][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 6},
                                     {6, 7}, {7, 8}, {8, 9}, {0, 9}, {10, 11}};
constexpr int kEvRing = 64;

struct HostLimiter {
    rl_limiter_config cfg;
    DevLimiter dev;
    void* table = nullptr;
    size_t table_bytes = 0;
    void* cache_table = nullptr;            // SW local cache: u64 per slot
};

inline int ceil_log2(uint64_t x) {
    int b = 0;
    while ((1ULL << b) < x) ++b;
    return b;
}

}  // namespace

// Per-batch scratch: the partition's records/positions, the [bin][tile] counts, the packed
// results and the batch control block. Two sets, so that with RL_OPT_PIPELINE the partition
// of batch k+1 (its own stream) can run while batch k's region stage still reads its set.
struct BatchScratch {
    size_t cap_n = 0;
    bool cap_wide = false;
    void* rec0 = nullptr;
    void* rec1 = nullptr;
    uint32_t* pos0 = nullptr;
    uint32_t* pos1 = nullptr;
    uint16_t* digit = nullptr;              // routing: pass-0 digit per request
    void* res = nullptr;
    int64_t* ext = nullptr;                 // escaped remainders (kResEscape), like res
    double* tok = nullptr;
    uint32_t* counts = nullptr;             // [bins][tiles]
    size_t counts_cap = 0;
    uint32_t* bin_total = nullptr;          // [2^kMaxDigitBits]
    uint32_t* bin_base = nullptr;           // [2^kMaxDigitBits]
    uint32_t* region_count = nullptr;       // [P padded]
    uint32_t* region_start = nullptr;
    size_t region_cap = 0;
    uint32_t* gtile = nullptr;              // k_group*: tile_base, tile_bin, per-tile counts
    size_t gtile_cap = 0;
    uint32_t* seg = nullptr;                // segmented pass 0: seg_adj, seg_start, seg_cnt
    size_t seg_cap = 0;
    BatchCtl* d_ctl = nullptr;
    hipEvent_t parted = nullptr;            // pipeline: partition done (partition stream)
    hipEvent_t freed = nullptr;             // pipeline: last reader of the set done (engine stream)
    bool used = false;                      // `freed` has been recorded
};

struct rl_engine {
    int device = 0;
    rl_opts opts{};
    int shard_bits = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;                          // one batch in flight per engine handle

    std::vector<HostLimiter> lims;
    uint32_t n_regions = 0;
    DevLimiter* d_lims = nullptr;
    uint8_t* d_region_lim = nullptr;
    size_t region_lim_cap = 0;

    // per-batch scratch (sized for opts.max_batch); sc[0] unless pipelined
    BatchScratch sc[2];
    int next_set = 0;
    bool pipeline = false;                  // RL_OPT_PIPELINE
    hipStream_t pstream = nullptr;          // partition stream (pipeline)
    hipEvent_t in_ev = nullptr;             // pipeline: inputs ready on e->stream
    hipStream_t hstream = nullptr;          // hot chains beside the normal regions
    hipEvent_t hot_ev[2] = {};              // fork, join of hstream
    // hot regions
    uint32_t* hot_list = nullptr;           // [kHotListWords]: list, k_hot_select's meta, totals
    HotInfo* hot_info = nullptr;            // [kHotMax]
    uint64_t* hot_summ = nullptr;           // [hot_summ_cap][8]
    size_t hot_summ_cap = 0, hot_summ_l1 = 0;
    uint2* walk_tab = nullptr;              // [kWalkTabEntries] allow-walk tables (hot chains)
    bool walk = true;                       // rl_tune("walk"): allow walks in the hot chains
    uint32_t walk_hint = 0;                 // listed regions that wanted a walk in the last batch
                                            // seen complete (walk_tab is allocated once it is > 0)
    uint32_t walk_min = kWalkMinAllows;     // rl_tune("walk_min"): fewest expected allows walked
    bool chain_split = true;                // rl_tune("chain_split"): two-wave hot chains
    uint32_t* hot_mark = nullptr;           // [hot_mark_cap] epoch marks per bin
    size_t hot_mark_cap = 0;
    uint32_t epoch = 0;
    uint32_t hot_threshold = 16384;         // rl_tune("hot_threshold"); 0 disables
    bool hot_thr_auto = true;               // until set: max(hot_threshold, n / 4096) per batch
    // Hot-region routing (two-pass batches): the previous batch's hot regions get pass-0 bins
    // of their own and skip pass 1. route_list holds region ids (kNone = unused); it is built
    // on device at the end of each batch's hot preparation and cleared when region ids change.
    bool route = true;                      // rl_tune("route")
    bool region_order = true;               // rl_tune("region_order"): largest regions dispatched first
    uint32_t order_prefix = 4096;           // rl_tune("order_prefix"): ... after this many of the smallest
    uint32_t tile_items = 0;                // rl_tune("tile_items"): partition tile rounds (0: auto)
    uint32_t segments = 1;                  // rl_tune("segments"): two-pass batches' pass-0 output
                                            // in that many tile segments ([segment][bin])
    uint32_t group_bits = 12;               // rl_tune("group_bits"): two-pass batches' pass-0
                                            // high digit (2^12 bins + the routed ones)
    uint32_t* order = nullptr;              // [order_cap + 1]
    size_t order_cap = 0;
    uint32_t* order_meta = nullptr;         // [kOrderMeta]
    // One table per scratch set: with RL_OPT_PIPELINE batch k+1's partition runs while batch
    // k's region stage still reads its routed ranges and writes the next table, so batch k uses
    // set k % 2's table, written by batch k - 2 (set 0 only without the option: batch k - 1).
    uint32_t* route_list = nullptr;         // [2][kRouteWords] region ids (kNone = empty), dense indices
    uint32_t* route_start = nullptr;        // [2][kRouteSlots] this batch's routed bins
    uint32_t* route_cnt = nullptr;          // [2][kRouteSlots]
    uint32_t solo_threshold = 4096;         // rl_tune("solo_threshold"): records per cache-on SW
                                            // region for the single-key allow-run pass (0: off)
    uint32_t* solo_list = nullptr;          // [kSoloMax + 1]: the listed regions, then their count
    uint32_t sparse_max = 96;               // rl_tune("sparse_max"): records per region up to
                                            // which a region probes single buckets; 0 = never
    uint64_t* dbg = nullptr;                // rl_tune("debug_regions"): per-bin stamps
    size_t dbg_cap = 0;
    bool debug_regions = false;
    unsigned long long* d_stats = nullptr;  // [kStatSlots][kStWords] sharded counters (zeroed)
    BatchCtl* h_ctl = nullptr;              // pinned copy of the last batch's ctl

    // host-API staging (device copies of caller buffers)
    size_t stage_cap = 0;
    uint64_t* s_key = nullptr;
    int32_t* s_permits = nullptr;
    int64_t* s_now = nullptr;
    uint16_t* s_lim = nullptr;
    uint8_t* s_op = nullptr;
    uint8_t* s_allowed = nullptr;
    int64_t* s_remaining = nullptr;
    double* s_tokens = nullptr;
    std::vector<std::pair<void*, size_t>> pinned;   // caller buffers registered by rl_pin_host

    // routing scratch
    uint32_t* route_scratch = nullptr;
    size_t route_cap = 0;
    uint32_t* route_counts = nullptr;
    DirSlot* d_dir = nullptr;               // hot-key owner directory (nullptr: hash owners)
    std::vector<DirSlot> h_dir;             // host copy (rl_owner_of_engine)

    hipEvent_t ev[kEvRing][kMarks] = {};
    int ring_used = 0;                      // batches recorded since the last query
    int ring_next = 0;
    bool timing = false;
    bool last_wide = false;
    bool pending_status = false;
    bool enqueued = false;                  // the last engine call enqueued a batch (d_ctl is its)
    uint32_t hot_hint = 0xFFFFFFFFu;        // hot regions of the last batch seen complete
    int last_status = RL_OK;
    uint64_t last_n = 0;
    uint32_t ablate = 0;                    // rl_tune("ablate"), measurement only
    uint32_t up_per_cu = 0, sc_per_cu = 0, un_per_cu = 0;   // rl_tune("*_per_cu"), 0 = default
    uint32_t sc_split = 1;                  // rl_tune("scatter_split"): k_scatter_split
    uint32_t un_split = 2;                  // rl_tune("unpermute_split"): k_unpermute_split
    uint32_t mid_xcd = 0;                   // rl_tune("mid_xcd"): k_unpermute_mid blocks XCD-aware (measured slower)
                                            // 0 off, 1 on, 2 two-pass batches (measured faster there)
    bool force_wide = false;                // rl_tune("wide_records"): 32-B records (any time span)
    bool auto_grow = true;                  // !RL_OPT_FIXED_CAPACITY
    uint32_t inject_fail = 0;               // rl_tune("fail_batches"): tests of callers' error paths
    uint64_t grows = 0;                     // region-count doublings done (rl_batch_stats)
    unsigned long long* retry_dbg = nullptr; // measurement builds (RL_RETRY_COUNT): k_retry_after's counters
    void* topk = nullptr;                   // rl_top_keys scratch (topk_scratch_bytes), on first use
    void* usage = nullptr;                  // rl_limiter_usage / rl_top_consumers scratch, on first use
    uint32_t usage_passes = 0;              // table passes of the last rl_top_consumers (rl_debug_fetch)
    BucketDigest* digest = nullptr;         // [digest_cap] the host form of rl_limiter_digest, largest so far
    size_t digest_cap = 0;
    BucketDigest* digest_fine = nullptr;    // [2^kDigestFineBits] the pass' output when fewer buckets are asked for
    uint32_t digest_per_cu = 0;             // rl_tune("digest_per_cu"), 0 = default
    void* snap = nullptr;                   // snapshot / ordered-put scratch (snap_scratch_bytes), on first use
    uint32_t* put_heads = nullptr;          // [put_heads_cap] run heads of an ordered put
    size_t put_heads_cap = 0;
    KeyImage* img_stage = nullptr;          // [img_stage_cap] images of rl_snapshot_keys / rl_restore_keys
    size_t img_stage_cap = 0;
    // string-key staging of rl_hash_keys / rl_execute_batch_keys, on first use
    size_t key_stage_bytes = (size_t)4 << 20;   // rl_tune("key_stage_bytes"): the blob stage's size
    uint8_t* ks_blob = nullptr;             // [ks_blob_cap] one chunk of key bytes
    size_t ks_blob_cap = 0;
    uint64_t* ks_off = nullptr;             // [ks_keys_cap + 1] offsets
    uint64_t* ks_hash = nullptr;            // [ks_keys_cap] rl_hash_keys' hashes
    unsigned long long* ks_hdr = nullptr;   // [2] the chunks' headers (the host checked the offsets)
    size_t ks_keys_cap = 0;
    bool keys_direct = false;               // rl_tune("keys_direct"): k_hash_keys' direct path only
};

#define HIP_OK(x)                                                      \
    do {                                                               \
        hipError_t _e = (x);                                           \
        if (_e != hipSuccess) {                                        \
            std::fprintf(stderr, "rl_engine: %s failed: %s (%s:%d)\n", #x, \
                         hipGetErrorString(_e), __FILE__, __LINE__);   \
            return RL_E_DEVICE;                                        \
        }                                                              \
    } while (0)

static void ensure_events(rl_engine* e) {
    if (e->ev[0][0]) return;
    for (int r = 0; r < kEvRing; ++r)
        for (int i = 0; i < kMarks; ++i) (void)hipEventCreate(&e->ev[r][i]);
}

static void dfree(void*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}
template <class T>
static void dfree(T*& p) {
    if (p) (void)hipFree((void*)p);
    p = nullptr;
}

static int dalloc(void** p, size_t bytes) {
    if (hipMalloc(p, bytes ? bytes : 16) != hipSuccess) {
        *p = nullptr;
        return RL_E_NOMEM;
    }
    return RL_OK;
}
template <class T>
static int dalloc(T** p, size_t count) {
    return dalloc((void**)p, count * sizeof(T));
}

// A temporary device allocation, freed with the scope that owns it.
template <class T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { dfree(p); }
    int alloc(size_t count) { return dalloc(&p, count); }
    operator T*() const { return p; }
};

// Orders the engine stream after the caller's work (construction; `err` says how that went)
// and the caller's stream after ours (finish(), or the destructor on an early return). Does
// nothing when the caller's stream is null or the engine's own.
struct StreamJoin {
    hipStream_t ours, user;
    hipEvent_t ev = nullptr;
    hipError_t err = hipSuccess;
    StreamJoin(hipStream_t ours_, hipStream_t user_) : ours(ours_), user(user_) {
        if (!user || user == ours) return;
        err = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (err != hipSuccess) { ev = nullptr; return; }
        err = hipEventRecord(ev, user);
        if (err == hipSuccess) err = hipStreamWaitEvent(ours, ev, 0);
    }
    StreamJoin(const StreamJoin&) = delete;
    StreamJoin& operator=(const StreamJoin&) = delete;
    hipError_t finish() {
        if (!ev) return hipSuccess;
        hipError_t he = hipEventRecord(ev, ours);
        if (he == hipSuccess) he = hipStreamWaitEvent(user, ev, 0);
        (void)hipEventDestroy(ev);
        ev = nullptr;
        return he;
    }
    ~StreamJoin() { (void)finish(); }
};

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
        if (rc == RL_OK) rc = dalloc(&B.d_ctl, 1);
        if (rc == RL_OK) rc = dalloc(&B.bin_total, 1u << kMaxDigitBits);
        if (rc == RL_OK) rc = dalloc(&B.bin_base, 1u << kMaxDigitBits);
        if (rc == RL_OK && e->pipeline &&
            (hipEventCreateWithFlags(&B.parted, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&B.freed, hipEventDisableTiming) != hipSuccess))
            rc = RL_E_DEVICE;
    }
    if (rc == RL_OK) rc = dalloc(&e->d_stats, (size_t)kStatSlots * kStWords);
    if (rc == RL_OK && hipMemset(e->d_stats, 0, (size_t)kStatSlots * kStWords * 8) != hipSuccess)
        rc = RL_E_DEVICE;
    if (rc == RL_OK && hipHostMalloc((void**)&e->h_ctl, sizeof(BatchCtl)) != hipSuccess) rc = RL_E_NOMEM;
    if (rc == RL_OK) rc = dalloc(&e->d_lims, RL_MAX_LIMITERS);
    if (rc == RL_OK) rc = dalloc(&e->hot_list, kHotListWords);
    if (rc == RL_OK) rc = dalloc(&e->hot_info, kHotMax);
    if (rc == RL_OK) rc = dalloc(&e->route_list, 2 * kRouteWords);
    if (rc == RL_OK) rc = dalloc(&e->route_start, 2 * kRouteSlots);
    if (rc == RL_OK) rc = dalloc(&e->route_cnt, 2 * kRouteSlots);
    if (rc == RL_OK) rc = dalloc(&e->order_meta, kOrderMeta);
    if (rc == RL_OK) rc = dalloc(&e->solo_list, kSoloMax + 1);
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
    dfree(e->d_lims); dfree(e->d_region_lim);
    for (BatchScratch& B : e->sc) {
        dfree(B.rec0); dfree(B.rec1); dfree(B.pos0); dfree(B.pos1); dfree(B.res); dfree(B.tok);
        dfree(B.ext); dfree(B.digit);
        dfree(B.counts); dfree(B.bin_total); dfree(B.bin_base);
        dfree(B.region_count); dfree(B.region_start); dfree(B.gtile); dfree(B.seg);
        dfree(B.d_ctl);
        if (B.parted) (void)hipEventDestroy(B.parted);
        if (B.freed) (void)hipEventDestroy(B.freed);
    }
    dfree(e->hot_list); dfree(e->hot_mark); dfree(e->dbg); dfree(e->hot_info); dfree(e->hot_summ);
    dfree(e->walk_tab);
    dfree(e->route_list); dfree(e->route_start); dfree(e->route_cnt);
    dfree(e->order); dfree(e->order_meta); dfree(e->solo_list);
    dfree(e->d_stats); dfree(e->retry_dbg); dfree(e->topk); dfree(e->usage); dfree(e->digest); dfree(e->digest_fine);
    dfree(e->snap); dfree(e->put_heads); dfree(e->img_stage);
    dfree(e->ks_blob); dfree(e->ks_off); dfree(e->ks_hash); dfree(e->ks_hdr);
    dfree(e->s_key); dfree(e->s_permits); dfree(e->s_now); dfree(e->s_lim); dfree(e->s_op);
    dfree(e->s_allowed); dfree(e->s_remaining); dfree(e->s_tokens);
    dfree(e->route_scratch); dfree(e->route_counts); dfree(e->d_dir);
    if (e->h_ctl) (void)hipHostFree(e->h_ctl);
    for (auto& pb : e->pinned) (void)hipHostUnregister(pb.first);
    for (int r = 0; r < kEvRing; ++r)
        for (int i = 0; i < kMarks; ++i) if (e->ev[r][i]) (void)hipEventDestroy(e->ev[r][i]);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    if (e->pstream) (void)hipStreamDestroy(e->pstream);
    if (e->in_ev) (void)hipEventDestroy(e->in_ev);
    if (e->hstream) (void)hipStreamDestroy(e->hstream);
    for (hipEvent_t ev : e->hot_ev) if (ev) (void)hipEventDestroy(ev);
    delete e;
}

static int upload_limiters(rl_engine* e) {
    std::vector<DevLimiter> dv;
    for (auto& l : e->lims) dv.push_back(l.dev);
    HIP_OK(hipMemcpy(e->d_lims, dv.data(), dv.size() * sizeof(DevLimiter), hipMemcpyHostToDevice));
    std::vector<uint8_t> map(e->n_regions);
    for (size_t li = 0; li < e->lims.size(); ++li) {
        const auto& d = e->lims[li].dev;
        std::fill(map.begin() + d.region_base, map.begin() + d.region_base + (1u << d.region_bits),
                  (uint8_t)li);
    }
    if (e->region_lim_cap < map.size()) {
        dfree(e->d_region_lim);
        if (dalloc(&e->d_region_lim, map.size()) != RL_OK) return RL_E_NOMEM;
        e->region_lim_cap = map.size();
    }
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
static int grow_once(rl_engine* e, size_t li) {
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

static int ensure_scratch(rl_engine* e, BatchScratch& B, size_t n, bool wide, uint32_t bins, uint32_t n_tiles) {
    if (n > B.cap_n || (wide && !B.cap_wide)) {
        // sized for this batch (+1/8 headroom), not max_batch: a router's engine accepts up
        // to its receive capacity but usually sees about its per-rank share
        size_t cap = std::max<size_t>(n, std::min<size_t>(e->opts.max_batch,
                                                          std::max<size_t>(n + n / 8, 1u << 20)));
        const size_t rb = wide ? sizeof(RecW) : sizeof(RecC);
        const size_t padn = cap + kTileThreads;   // kernels write inactive lanes past n
        dfree(B.rec0); dfree(B.rec1); dfree(B.pos0); dfree(B.pos1); dfree(B.res); dfree(B.tok);
        dfree(B.ext); dfree(B.digit);
        int rc = dalloc(&B.rec0, padn * rb);
        if (rc == RL_OK) rc = dalloc(&B.digit, padn);
        if (rc == RL_OK) rc = dalloc(&B.rec1, padn * rb);
        if (rc == RL_OK) rc = dalloc(&B.pos0, padn);
        if (rc == RL_OK) rc = dalloc(&B.pos1, padn);
        if (rc == RL_OK) rc = dalloc(&B.res, padn * sizeof(uint64_t));
        if (rc == RL_OK) rc = dalloc(&B.tok, padn);
        if (rc == RL_OK) rc = dalloc(&B.ext, padn);
        if (rc != RL_OK) { B.cap_n = 0; return rc; }
        B.cap_n = cap;
        B.cap_wide = wide;
    }
    const size_t need_counts = (size_t)bins * n_tiles;
    if (need_counts > B.counts_cap) {
        dfree(B.counts);
        size_t c = std::max(need_counts, (size_t)(1u << kMaxDigitBits) *
                                              ((std::max<size_t>(n, B.cap_n) + kTile - 1) / kTile));
        if (dalloc(&B.counts, c) != RL_OK) return RL_E_NOMEM;
        B.counts_cap = c;
    }
    return RL_OK;
}

// rstart / rend per region for two-pass partitions (k_group).
static int ensure_regions(BatchScratch& B, size_t bins) {
    if (bins <= B.region_cap) return RL_OK;
    dfree(B.region_count); dfree(B.region_start);
    int rc = dalloc(&B.region_count, bins);
    if (rc == RL_OK) rc = dalloc(&B.region_start, bins);
    if (rc != RL_OK) { B.region_cap = 0; return rc; }
    B.region_cap = bins;
    return RL_OK;
}

// chunk summaries [l1] then group summaries [l1 / 64 + kHotMax + 1], 64 B each (two keys)
static int ensure_hot_summ(rl_engine* e, size_t n) {
    const size_t l1 = n / kHotChunk + kHotMax + 1;
    const size_t need = l1 + l1 / 64 + kHotMax + 1;
    if (need <= e->hot_summ_cap) return RL_OK;
    dfree(e->hot_summ);
    if (dalloc(&e->hot_summ, need * 8) != RL_OK) { e->hot_summ_cap = 0; return RL_E_NOMEM; }
    e->hot_summ_cap = need;
    e->hot_summ_l1 = l1;
    return RL_OK;
}

static int ensure_hot_mark(rl_engine* e, size_t bins) {
    if (bins <= e->hot_mark_cap) return RL_OK;
    dfree(e->hot_mark);
    if (dalloc(&e->hot_mark, bins) != RL_OK) { e->hot_mark_cap = 0; return RL_E_NOMEM; }
    HIP_OK(hipMemset(e->hot_mark, 0, bins * sizeof(uint32_t)));
    e->hot_mark_cap = bins;
    e->epoch = 0;
    return RL_OK;
}

static inline void mark_on(rl_engine* e, hipStream_t st, int i) {
    if (e->timing) (void)hipEventRecord(e->ev[e->ring_next][i], st);
}
static inline void mark(rl_engine* e, int i) { mark_on(e, e->stream, i); }

// The pipeline on device buffers, enqueued on e->stream. Returns an immediate status
// (argument/launch errors); the data-dependent status is read back by rl_last_status.
static int run_batch_device(rl_engine* e, size_t n, const uint64_t* key, const int32_t* permits,
                            const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op,
                            uint8_t* allowed, int64_t* remaining, double* tokens_after,
                            bool overlap = false) {
    if (n > e->opts.max_batch) return RL_E_TOO_LARGE;
    e->last_n = n;
    e->pending_status = false;
    e->enqueued = false;
    e->last_status = RL_OK;
    if (n == 0) return RL_OK;
    if (!key || !permits || !now_ns || !allowed || !remaining) return RL_E_INVALID_ARG;
    if (e->inject_fail) { --e->inject_fail; return RL_E_DEVICE; }   // nothing enqueued
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
    // partition tiles of 128K requests for large batches (half the [bin][tile] counts to write
    // and scan: sw_zipf's 2^28-request batches, scan0 0.16 -> 0.06 ms, upsweep0 0.89 -> 0.75 ms),
    // 64K below (tb_uniform's 2^26 needs the 1024 tiles to keep every CU busy; the unpermute keeps
    // 64K tiles: run_r06o.sh)
    const uint32_t titems = e->tile_items ? e->tile_items
                                          : (n >= ((size_t)3 << 26) ? 2u * kTileItems : (uint32_t)kTileItems);
    const size_t tile_n = (size_t)titems * kTileThreads;
    const uint32_t nt = (uint32_t)((n + tile_n - 1) / tile_n);
    const uint32_t nt_un = (uint32_t)((n + kTile - 1) / kTile);
    bool cache = false;
    for (auto& l : e->lims) cache |= l.dev.cache_ttl_ms > 0;
    const uint32_t n_bins = e->n_regions;            // one partition bin per region
    const int bitsP = std::max(1, ceil_log2(n_bins));
    const int passes = bitsP <= kMaxDigitBits ? 1 : 2;
    if (bitsP > 2 * kMaxDigitBits) return RL_E_LIMITERS;
    // Two passes: pass 0 partitions by the high dh bits of the region id (2^dh bins of 2^s0
    // consecutive regions), then k_group groups each bin by region locally (rl_partition.hip)
    const int dh = passes == 1 ? bitsP
                               : std::max(bitsP - kMaxDigitBits, std::min<int>((int)e->group_bits, kMaxDigitBits));
    const int s0 = bitsP - dh;
    // hot-region routing: pass 0 gets kRouteBins dense bins beyond the 2^dh high-digit ones. The
    // hot path is gated per limiter: regions of a limiter with the local cache are never
    // listed hot (k_hot_select), so they are never routed either; the other limiters keep it.
    const bool hot_on = e->hot_threshold > 0;
    const bool route = hot_on && e->route && passes == 2 &&
                       (1u << dh) + kRouteBins <= (1u << kMaxDigitBits);
    const uint32_t nb0 = route ? (1u << dh) + kRouteBins : 1u << dh;
    // segmented pass-0 output (two passes): n_segs runs of seg_tiles tiles
    const uint32_t seg_tiles = passes == 2 && e->segments > 1 ? (nt + e->segments - 1) / e->segments : nt;
    const uint32_t n_segs = (nt + seg_tiles - 1) / seg_tiles;
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
    const size_t need_counts = (size_t)nb0 * nt;
    if (e->pipeline && (n > B.cap_n || (wide && !B.cap_wide) || need_counts > B.counts_cap ||
                        (passes == 2 && n_bins > B.region_cap))) {
        // growing a set frees its old buffers: nothing may still be using them
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipStreamSynchronize(ps));
    }
    int rc = ensure_scratch(e, B, n, wide, nb0, nt);
    if (rc != RL_OK) return rc;
    if (passes == 2) {
        rc = ensure_regions(B, n_bins);
        if (rc != RL_OK) return rc;
    }
    if (e->pipeline) {
        if (B.used) HIP_OK(hipStreamWaitEvent(ps, B.freed, 0));    // the set's last batch is done
        if (!overlap) {
            HIP_OK(hipEventRecord(e->in_ev, s));
            HIP_OK(hipStreamWaitEvent(ps, e->in_ev, 0));
        }
    }
    const bool hot = hot_on;
    // records per region for the hot path: scaled with the batch by default (measured per
    // config: sw_zipf best at 65536 for 2^28 requests, zipf_1b at 32768 for 2^27)
    const uint32_t hot_thr = e->hot_thr_auto ? std::max<uint32_t>(e->hot_threshold, (uint32_t)(n >> 12))
                                             : e->hot_threshold;
    if (hot) {
        rc = ensure_hot_mark(e, n_bins);
        if (rc == RL_OK) rc = ensure_hot_summ(e, n);
        if (rc != RL_OK) return rc;
        // Allow-walk tables (512 MiB): only once a batch had a key dense enough to walk
        // (k_hot_scan's count; a workload that never walks, such as tb_uniform, holds none).
        // The walk is optional and decides identically: a failed allocation turns it off.
        if (e->walk && !e->walk_tab && e->walk_hint > 0 && dalloc(&e->walk_tab, kWalkTabEntries) != RL_OK) {
            std::fprintf(stderr, "rl_engine: no device memory for the allow-walk tables; walks off\n");
            e->walk = false;
        }
        if (++e->epoch == 0) {                       // marks hold epochs: restart after wrap
            HIP_OK(hipMemsetAsync(e->hot_mark, 0, e->hot_mark_cap * sizeof(uint32_t), s));
            e->epoch = 1;
        }
    }
    e->last_wide = wide;

    mark_on(e, ps, 0);
    PartArgs pa{};
    pa.key = key; pa.permits = permits; pa.now_ns = now_ns; pa.limiter = limiter; pa.op = op;
    pa.n = (uint32_t)n; pa.n_tiles = nt; pa.tile_items = titems; pa.n_lim = (uint32_t)e->lims.size();
    pa.shard_bits = e->shard_bits; pa.lims = e->d_lims; pa.ctl = B.d_ctl;
    pa.counts = B.counts; pa.bin_base = B.bin_base; pa.ablate = e->ablate;
    // (128K-request tiles: one upsweep tile per workgroup, 8 per CU: upsweep0 0.76 -> 0.73 ms on
    // sw_zipf over 6 runs, run_r06ab.sh)
    pa.up_per_cu = e->up_per_cu ? e->up_per_cu : (titems > (uint32_t)kTileItems ? 8u : 0u);
    pa.sc_per_cu = e->sc_per_cu; pa.sc_split = e->sc_split;
    // ---- pass 0 (the high digit: region >> s0) from the caller's arrays; routed hot
    // regions get bins 2^dh + slot and their records go straight to the final array (rec1)
    pa.digit_shift = s0; pa.digit_bits = route ? ceil_log2(nb0) : dh;
    pa.n_bins_pass = nb0;
    pa.rec_out = passes == 2 ? B.rec0 : B.rec1; pa.pos_out = B.pos0;
    if (route) {
        pa.route_list = r_list; pa.lo_bins = 1u << dh; pa.rec_out_route = B.rec1;
        pa.digit = B.digit;
    }
    HIP_OK(launch_upsweep(pa, true, wide, ps));
    mark_on(e, ps, 1);
    HIP_OK(launch_scan_rows(B.counts, B.counts, nb0, nt, B.bin_total, ps));
    HIP_OK(launch_scan_small(B.bin_total, B.bin_base, nb0, ps));
    if (n_segs > 1) {
        const size_t words = (size_t)3 * nb0 * n_segs;
        if (words > B.seg_cap) {
            if (e->pipeline) { HIP_OK(hipStreamSynchronize(s)); HIP_OK(hipStreamSynchronize(ps)); }
            dfree(B.seg);
            if (dalloc(&B.seg, words) != RL_OK) { B.seg_cap = 0; return RL_E_NOMEM; }
            B.seg_cap = words;
        }
        const size_t m = (size_t)nb0 * n_segs;
        HIP_OK(launch_seg_base(B.counts, B.bin_total, B.bin_base, nb0, 1u << dh, nt, seg_tiles, n_segs,
                               B.seg, B.seg + m, B.seg + 2 * m, ps));
        pa.seg_adj = B.seg; pa.n_segs = n_segs; pa.seg_tiles = seg_tiles;
    }
    mark_on(e, ps, 2);
    HIP_OK(launch_scatter(pa, true, wide, ps));
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
        ga.tile_recs = group_tile_recs((uint32_t)s0);
        ga.pad = (uint32_t)n;
        ga.ablate = e->ablate;
        ga.max_tiles = (uint32_t)((n + ga.tile_recs - 1) / ga.tile_recs) + ga.n_bins0 * n_segs;
        const size_t words = (size_t)ga.n_bins0 + 1 + (size_t)ga.max_tiles * (1 + ((size_t)1 << s0)) +
                             (n_segs > 1 ? (size_t)2 * ga.max_tiles : 0);
        if (words > B.gtile_cap) {
            if (e->pipeline) { HIP_OK(hipStreamSynchronize(s)); HIP_OK(hipStreamSynchronize(ps)); }
            dfree(B.gtile);
            if (dalloc(&B.gtile, words) != RL_OK) { B.gtile_cap = 0; return RL_E_NOMEM; }
            B.gtile_cap = words;
        }
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
        if (e->dbg_cap < (size_t)n_bins * kDbgWords) {
            dfree(e->dbg);
            if (dalloc(&e->dbg, (size_t)n_bins * kDbgWords) != RL_OK) { e->dbg_cap = 0; return RL_E_NOMEM; }
            e->dbg_cap = (size_t)n_bins * kDbgWords;
        }
        HIP_OK(hipMemsetAsync(e->dbg, 0, e->dbg_cap * sizeof(uint64_t), s));
        ra.dbg = e->dbg;
    }
    if (hot) {
        uint32_t* hot_count = e->hot_list + kHotMax;
        HIP_OK(hipMemsetAsync(hot_count, 0, kHotMetaWords * sizeof(uint32_t), s));
        if (route) HIP_OK(launch_hot_route_list(r_list, r_cnt, e->hot_list, hot_count, s));
        HIP_OK(launch_hot_select(rstart, rcount, rend, n_bins, hot_thr, e->hot_list,
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
        if (e->order_cap < n_bins) {
            dfree(e->order);
            if (dalloc(&e->order, (size_t)n_bins + 1) != RL_OK) { e->order_cap = 0; return RL_E_NOMEM; }
            e->order_cap = n_bins;
        }
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
    if (hot && e->route && passes == 2)
        HIP_OK(launch_route_next(e->hot_info, e->hot_list + kHotMax, hot_thr, r_list, s));
    HIP_OK(launch_stats_reduce(e->d_stats, B.d_ctl, s));
    mark(e, 11);
    mark(e, 8);
    UnpermArgs ua{};
    ua.pos0 = B.pos0; ua.pos1 = passes == 2 ? B.pos1 : nullptr; ua.res = B.res;
    ua.mid = B.rec0;                                    // pass-0 records are dead by now
    ua.tok = tokens_after ? B.tok : nullptr;
    ua.ext = B.ext; ua.ctl = B.d_ctl;
    ua.allowed = allowed; ua.remaining = remaining; ua.tokens_out = tokens_after;
    ua.n = (uint32_t)n; ua.n_tiles = nt_un; ua.ablate = e->ablate; ua.per_cu = e->un_per_cu;
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

static int collect_status(rl_engine* e) {
    HIP_OK(hipStreamSynchronize(e->stream));
    if (e->pstream) HIP_OK(hipStreamSynchronize(e->pstream));
    if (!e->pending_status) return e->last_status;
    e->pending_status = false;
    BatchCtl& c = *e->h_ctl;
    e->hot_hint = c.n_hot;
    e->walk_hint = c.n_walk;
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

extern "C" int rl_execute_batch_device(rl_engine* e, size_t n, const uint64_t* key,
                                       const int32_t* permits, const int64_t* now_ns,
                                       const uint16_t* limiter, const uint8_t* op,
                                       uint8_t* allowed, int64_t* remaining, double* tokens_after,
                                       void* stream) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    hipStream_t user = (hipStream_t)stream;
    if (user && user != e->stream) {
        // order the engine stream after the caller's work, and the caller's after ours
        hipEvent_t ev;
        HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_OK(hipEventRecord(ev, user));
        HIP_OK(hipStreamWaitEvent(e->stream, ev, 0));
        int rc = run_batch_device(e, n, key, permits, now_ns, limiter, op, allowed, remaining,
                                  tokens_after);
        HIP_OK(hipEventRecord(ev, e->stream));
        HIP_OK(hipStreamWaitEvent(user, ev, 0));
        (void)hipEventDestroy(ev);
        return rc;
    }
    return run_batch_device(e, n, key, permits, now_ns, limiter, op, allowed, remaining,
                            tokens_after, /*overlap=*/user == nullptr);
}

extern "C" int rl_last_status(rl_engine* e) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    return collect_status(e);
}

static int ensure_staging(rl_engine* e, size_t n) {
    if (n <= e->stage_cap) return RL_OK;
    dfree(e->s_key); dfree(e->s_permits); dfree(e->s_now); dfree(e->s_lim); dfree(e->s_op);
    dfree(e->s_allowed); dfree(e->s_remaining); dfree(e->s_tokens);
    int rc = dalloc(&e->s_key, n);
    if (rc == RL_OK) rc = dalloc(&e->s_permits, n);
    if (rc == RL_OK) rc = dalloc(&e->s_now, n);
    if (rc == RL_OK) rc = dalloc(&e->s_lim, n);
    if (rc == RL_OK) rc = dalloc(&e->s_op, n);
    if (rc == RL_OK) rc = dalloc(&e->s_allowed, n);
    if (rc == RL_OK) rc = dalloc(&e->s_remaining, n);
    if (rc == RL_OK) rc = dalloc(&e->s_tokens, n);
    if (rc != RL_OK) { e->stage_cap = 0; return rc; }
    e->stage_cap = n;
    return RL_OK;
}

// The host-buffer calls' requests into the staging arrays (limiter, op_or_skip: nullable; key
// null: s_key is filled by the caller, rl_execute_batch_keys).
static int stage_requests(rl_engine* e, size_t n, const uint64_t* key, const int32_t* permits,
                          const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op_or_skip) {
    const int rc = ensure_staging(e, n);
    if (rc != RL_OK) return rc;
    hipStream_t s = e->stream;
    if (key) HIP_OK(hipMemcpyAsync(e->s_key, key, n * 8, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(e->s_permits, permits, n * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(e->s_now, now_ns, n * 8, hipMemcpyHostToDevice, s));
    if (limiter) HIP_OK(hipMemcpyAsync(e->s_lim, limiter, n * 2, hipMemcpyHostToDevice, s));
    if (op_or_skip) HIP_OK(hipMemcpyAsync(e->s_op, op_or_skip, n, hipMemcpyHostToDevice, s));
    return RL_OK;
}

// The staged batch (stage_requests) run, collected and copied back: the body of the host-buffer
// batch calls.
static int run_staged_batch(rl_engine* e, size_t n, bool limiter, bool op, uint8_t* allowed,
                            int64_t* remaining, double* tokens_after) {
    hipStream_t s = e->stream;
    int rc = run_batch_device(e, n, e->s_key, e->s_permits, e->s_now, limiter ? e->s_lim : nullptr,
                              op ? e->s_op : nullptr, e->s_allowed, e->s_remaining,
                              tokens_after ? e->s_tokens : nullptr);
    if (rc != RL_OK) { (void)hipStreamSynchronize(s); return rc; }
    rc = collect_status(e);
    if (rc == RL_E_INVALID_ARG && e->h_ctl->span_overflow && !e->force_wide) {
        // the batch spans more than the compact record's 2^32 ms: it was rejected before any
        // state was touched, so run it again in 32-B records (full now_ms)
        e->force_wide = true;
        rc = run_batch_device(e, n, e->s_key, e->s_permits, e->s_now, limiter ? e->s_lim : nullptr,
                              op ? e->s_op : nullptr, e->s_allowed, e->s_remaining,
                              tokens_after ? e->s_tokens : nullptr);
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
    int rc = stage_requests(e, n, key, permits, now_ns, limiter, op);
    if (rc != RL_OK) return rc;
    return run_staged_batch(e, n, limiter != nullptr, op != nullptr, allowed, remaining, tokens_after);
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

// ---------------------------------------------------------------- retry-after queries
// One launch of k_retry_after on the engine stream: behind every batch submitted before it
// (the decision stage, the hot chains' side stream and the unpermute all run on or are joined
// on e->stream, with RL_OPT_PIPELINE too: only a batch's partition runs elsewhere). It reads
// the limiter table as uploaded by the last growth and touches no batch scratch, statistic or
// status word.
static int run_retry_device(rl_engine* e, size_t n, const uint64_t* key, const int32_t* permits,
                            const int64_t* now_ns, const uint16_t* limiter, const uint8_t* skip,
                            int64_t* wait_ms) {
    RetryArgs ra{};
    ra.key = key; ra.permits = permits; ra.now_ns = now_ns; ra.limiter = limiter; ra.skip = skip;
    ra.wait_ms = wait_ms;
    ra.lims = e->d_lims; ra.n = (uint32_t)n; ra.n_lim = (uint32_t)e->lims.size();
    ra.shard_bits = e->shard_bits;
#ifdef RL_RETRY_COUNT
    if (!e->retry_dbg) {
        if (dalloc(&e->retry_dbg, 3) != RL_OK) return RL_E_NOMEM;
        HIP_OK(hipMemset(e->retry_dbg, 0, 3 * sizeof(unsigned long long)));
    }
    ra.dbg = e->retry_dbg;
#endif
    HIP_OK(launch_retry_after(ra, e->stream));
    return RL_OK;
}

extern "C" int rl_retry_after_device(rl_engine* e, size_t n, const uint64_t* key_hash,
                                     const int32_t* permits, const int64_t* now_ns,
                                     const uint16_t* limiter, const uint8_t* skip,
                                     int64_t* wait_ms, void* stream) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (n > e->opts.max_batch) return RL_E_TOO_LARGE;
    if (n == 0) return RL_OK;
    if (!key_hash || !permits || !now_ns || !wait_ms) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    StreamJoin join(e->stream, (hipStream_t)stream);
    HIP_OK(join.err);
    const int rc = run_retry_device(e, n, key_hash, permits, now_ns, limiter, skip, wait_ms);
    HIP_OK(join.finish());
    return rc;
}

extern "C" int rl_retry_after(rl_engine* e, size_t n, const uint64_t* key_hash, const int32_t* permits,
                              const int64_t* now_ns, const uint16_t* limiter, const uint8_t* skip,
                              int64_t* wait_ms) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (n > e->opts.max_batch) return RL_E_TOO_LARGE;
    if (n == 0) return RL_OK;
    if (!key_hash || !permits || !now_ns || !wait_ms) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    // as the host-buffer batch calls: the last batch's status is collected first, which applies
    // the table growth it asked for (rl_last_status returns that same status afterwards)
    const int st = collect_status(e);
    if (st == RL_E_DEVICE) return st;
    int rc = stage_requests(e, n, key_hash, permits, now_ns, limiter, skip);
    if (rc != RL_OK) return rc;
    hipStream_t s = e->stream;
    rc = run_retry_device(e, n, e->s_key, e->s_permits, e->s_now, limiter ? e->s_lim : nullptr,
                          skip ? e->s_op : nullptr, e->s_remaining);
    if (rc != RL_OK) { (void)hipStreamSynchronize(s); return rc; }
    HIP_OK(hipMemcpyAsync(wait_ms, e->s_remaining, n * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i)
        if (wait_ms[i] == RL_RETRY_INVALID) return RL_E_INVALID_REQUEST;
    return RL_OK;
}

// ---------------------------------------------------------------- heavy-hitter keys
// rl_topk.hip on the engine stream: clear, the sketch pass and the filter pass over the keys
// (the host form: over every staged chunk), compact + select. Nothing here touches a limiter
// table, the batch scratch, d_stats, d_ctl or the status bookkeeping.
static_assert(RL_TOP_KEYS_MAX == kTopkMax && RL_TOP_KEYS_MAX == kDirMax, "top keys = directory capacity");
static_assert(RL_TOP_KEYS_CANDIDATES == kTopkCandidates, "candidate cap");
constexpr uint64_t kTopkMaxN = 1ULL << 31;

static bool topk_args_ok(rl_engine* e, size_t n, const uint64_t* key_hash, uint32_t k, uint64_t min_count) {
    return e && (n == 0 || key_hash) && k != 0 && k <= RL_TOP_KEYS_MAX && min_count != 0 &&
           (uint64_t)n <= kTopkMaxN;
}

static int topk_scratch(rl_engine* e, TopkScratch* sc) {
    if (!e->topk) {
        int rc = dalloc(&e->topk, topk_scratch_bytes());
        if (rc != RL_OK) return rc;
    }
    *sc = topk_scratch_at(e->topk);
    return RL_OK;
}

extern "C" int rl_top_keys_device(rl_engine* e, size_t n, const uint64_t* key_hash, uint32_t k,
                                  uint64_t min_count, uint64_t* top_key, uint64_t* top_count,
                                  uint64_t* hdr, void* stream) {
    if (!topk_args_ok(e, n, key_hash, k, min_count) || !top_key || !top_count || !hdr)
        return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    TopkScratch sc;
    int rc = topk_scratch(e, &sc);
    if (rc != RL_OK) return rc;
    hipStream_t s = e->stream;
    StreamJoin join(s, (hipStream_t)stream);
    HIP_OK(join.err);
    HIP_OK(launch_topk_clear(sc, s));
    HIP_OK(launch_topk_pass(sc, 0, key_hash, (uint32_t)n, min_count, s));
    HIP_OK(launch_topk_pass(sc, 1, key_hash, (uint32_t)n, min_count, s));
    HIP_OK(launch_topk_select(sc, k, min_count, n, top_key, top_count, hdr, s));
    HIP_OK(join.finish());
    return RL_OK;
}

extern "C" int rl_top_keys(rl_engine* e, size_t n, const uint64_t* key_hash, uint32_t k,
                           uint64_t min_count, uint64_t* top_key, uint64_t* top_count, size_t* n_out,
                           uint64_t* n_heavy) {
    if (!topk_args_ok(e, n, key_hash, k, min_count) || !top_key || !top_count || !n_out || !n_heavy)
        return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    TopkScratch sc;
    int rc = topk_scratch(e, &sc);
    if (rc != RL_OK) return rc;
    // chunks of the staging buffers' size (at most max_batch keys, as the batch calls leave
    // them); every chunk is uploaded once per pass
    const size_t chunk = std::min<size_t>(std::max<size_t>(n, 1), (size_t)e->opts.max_batch);
    rc = ensure_staging(e, chunk);
    if (rc != RL_OK) return rc;
    hipStream_t s = e->stream;
    HIP_OK(launch_topk_clear(sc, s));
    for (int pass = 0; pass < 2; ++pass)
        for (size_t at = 0; at < n; at += chunk) {
            const size_t m = std::min(chunk, n - at);
            HIP_OK(hipMemcpyAsync(e->s_key, key_hash + at, m * 8, hipMemcpyHostToDevice, s));
            HIP_OK(launch_topk_pass(sc, pass, e->s_key, (uint32_t)m, min_count, s));
        }
    HIP_OK(launch_topk_select(sc, k, min_count, n, sc.out_key, sc.out_cnt, sc.out_hdr, s));
    uint64_t hdr[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(hdr, sc.out_hdr, sizeof(hdr), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    *n_out = 0;
    *n_heavy = 0;
    if (hdr[2]) return RL_E_CAPACITY;
    if (hdr[0] > k) return RL_E_INTERNAL;
    if (hdr[0]) {
        HIP_OK(hipMemcpy(top_key, sc.out_key, hdr[0] * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(top_count, sc.out_cnt, hdr[0] * 8, hipMemcpyDeviceToHost));
    }
    *n_out = (size_t)hdr[0];
    *n_heavy = hdr[1];
    return RL_OK;
}

// ---------------------------------------------------------------- census of a limiter's table
// rl_usage.hip on the engine stream, behind every batch submitted before (as rl_export_state:
// the decision stage and the unpermute run on or are joined on e->stream, with RL_OPT_PIPELINE
// too). Both calls read the table as installed (no collect_status: a growth the last batch asked
// for is not applied, its status stays uncollected) and touch no limiter state, batch scratch,
// d_stats, d_ctl or status word.
static_assert(RL_USAGE_BINS == kUsageBins, "histogram bins");
static_assert(RL_USAGE_CANDIDATES == kUsageCandidates, "candidate cap");
static_assert(sizeof(rl_usage) == 8 * (7 + RL_USAGE_BINS), "rl_usage layout");

static int usage_scratch(rl_engine* e, UsageScratch* sc) {
    if (!e->usage) {
        int rc = dalloc(&e->usage, usage_scratch_bytes());
        if (rc != RL_OK) return rc;
    }
    *sc = usage_scratch_at(e->usage);
    return RL_OK;
}

extern "C" int rl_limiter_usage(rl_engine* e, uint16_t limiter, int64_t now_ns, rl_usage* out) {
    if (!e || !out) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    UsageScratch sc;
    int rc = usage_scratch(e, &sc);
    if (rc != RL_OK) return rc;
    const HostLimiter& h = e->lims[limiter];
    const uint64_t n_slots = h.table_bytes / sizeof(Slot);
    hipStream_t s = e->stream;
    unsigned long long c[kUcWords];
    HIP_OK(hipMemsetAsync(sc.counters, 0, 32 * sizeof(unsigned long long), s));
    HIP_OK(launch_usage_census(sc, (const Slot*)h.table, n_slots, h.dev, floor_div_ms(now_ns), s));
    HIP_OK(hipMemcpyAsync(c, sc.counters, sizeof(c), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    out->slots = n_slots;
    out->used_slots = c[kUcUsedSlots];
    out->live_keys = c[kUcLive];
    out->redis_keys = c[kUcRedis];
    out->exhausted_keys = c[kUcExhausted];
    out->cache_blocked = c[kUcCacheBlocked];
    out->used_permits = c[kUcUsedPermits];
    for (uint32_t b = 0; b < kUsageBins; ++b) out->hist[b] = c[kUcHist + b];
    return RL_OK;
}

// MSD radix select over C = used << 64 | ~key_hash (largest first = used descending, key_hash
// ascending): every pass histograms the next 12-bit digit of the keys that match the prefix
// chosen so far, the host picks the digit in which the k-th key lies, and refinement stops as
// soon as that cut bin holds at most RL_USAGE_CANDIDATES keys (or no bit is left: one key).
// The compaction then fetches the cut bin and the fewer than k keys above it, ordered here.
extern "C" int rl_top_consumers(rl_engine* e, uint16_t limiter, int64_t now_ns, uint32_t k,
                                int64_t min_used, uint64_t* key_hash, int64_t* used, size_t* n_out,
                                uint64_t* n_match) {
    if (!e || !key_hash || !used || !n_out || !n_match || k == 0 || k > RL_TOP_KEYS_MAX || min_used < 0)
        return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    UsageScratch sc;
    int rc = usage_scratch(e, &sc);
    if (rc != RL_OK) return rc;
    const HostLimiter& h = e->lims[limiter];
    const uint64_t n_slots = h.table_bytes / sizeof(Slot);
    const int64_t now = floor_div_ms(now_ns);
    hipStream_t s = e->stream;
    uint32_t ubits = 0;                              // bit_length(max_permits): used <= max_permits
    while (ubits < 63 && ((uint64_t)h.dev.max_permits >> ubits) != 0) ++ubits;
    UsageSel sel{};
    sel.min_used = min_used;
    sel.top = ubits + 64;
    unsigned __int128 prefix = 0;
    std::vector<unsigned long long> hist(kUsageDigits);
    uint64_t matched = 0, need = 0, keep = 0, cut_count = 0;
    e->usage_passes = 0;
    for (bool first = true;; first = false) {
        const uint32_t width = std::min<uint32_t>(kUsageDigitBits, sel.top);
        sel.pos = sel.top - width;
        sel.prefix_hi = (uint64_t)(prefix >> 64);
        sel.prefix_lo = (uint64_t)prefix;
        HIP_OK(hipMemsetAsync(sc.hist, 0, kUsageDigits * sizeof(unsigned long long), s));
        HIP_OK(launch_usage_digits(sc, (const Slot*)h.table, n_slots, h.dev, now, sel, s));
        HIP_OK(hipMemcpyAsync(hist.data(), sc.hist, kUsageDigits * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        e->usage_passes += 1;
        if (first) {
            for (uint32_t b = 0; b < (1u << width); ++b) matched += hist[b];
            if (matched == 0) {
                *n_out = 0;
                *n_match = 0;
                return RL_OK;
            }
            keep = need = std::min<uint64_t>(k, matched);
        }
        // the digit that holds the need-th largest of the keys under the prefix
        uint64_t above = 0;
        uint32_t cut = (1u << width) - 1;
        for (;; --cut) {
            if (above + hist[cut] >= need) break;
            above += hist[cut];
            if (cut == 0) return RL_E_INTERNAL;      // (the bins sum to the previous cut bin >= need)
        }
        need -= above;
        cut_count = hist[cut];
        prefix = (prefix << width) | cut;
        sel.top = sel.pos;
        if (cut_count <= kUsageCandidates || sel.top == 0) break;
    }
    sel.prefix_hi = (uint64_t)(prefix >> 64);
    sel.prefix_lo = (uint64_t)prefix;
    const uint64_t expect = (keep - need) + cut_count;   // the keys above the cut bin, and the bin
    if (expect > kUsageStore) return RL_E_INTERNAL;
    unsigned long long got = 0;
    HIP_OK(hipMemsetAsync(sc.counters + kUsageCandCount, 0, sizeof(unsigned long long), s));
    HIP_OK(launch_usage_compact(sc, (const Slot*)h.table, n_slots, h.dev, now, sel, s));
    HIP_OK(hipMemcpyAsync(&got, sc.counters + kUsageCandCount, sizeof(got), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    e->usage_passes += 1;
    if (got != expect) return RL_E_INTERNAL;
    std::vector<UsageCand> cand(got);
    HIP_OK(hipMemcpy(cand.data(), sc.cand, got * sizeof(UsageCand), hipMemcpyDeviceToHost));
    std::partial_sort(cand.begin(), cand.begin() + (long)keep, cand.end(),
                      [](const UsageCand& x, const UsageCand& y) {
                          return x.used != y.used ? x.used > y.used : x.key_hash < y.key_hash;
                      });
    for (uint64_t i = 0; i < keep; ++i) {
        key_hash[i] = cand[i].key_hash;
        used[i] = cand[i].used;
    }
    *n_out = (size_t)keep;
    *n_match = matched;
    return RL_OK;
}

// ---------------------------------------------------------------- string keys
// rl_keys.hip on the engine stream. The hash calls touch no limiter table, batch scratch,
// d_stats, d_ctl or the status bookkeeping; rl_execute_batch_keys hashes into s_key and then
// runs the batch as rl_execute_batch does.
static_assert(RL_KEY_MAX_BYTES == kKeyMaxBytes, "key length limit");
constexpr uint64_t kKeysMaxN = 1ULL << 31;

extern "C" uint64_t rl_key_hash(const void* bytes, size_t len) {
    const unsigned char* b = (const unsigned char*)bytes;
    uint64_t h = kFnvOffset;
    for (size_t i = 0; i < len; ++i) h = (h ^ b[i]) * kFnvPrime;
    return mix64(h);
}

static int hash_keys_enqueue(rl_engine* e, size_t n, const uint8_t* bytes, uint64_t bytes_len,
                             const uint64_t* off, uint64_t bias, uint64_t* out, unsigned long long* hdr) {
    HIP_OK(hipMemsetAsync(hdr, 0, 2 * sizeof(uint64_t), e->stream));
    KeysArgs a{};
    a.bytes = bytes; a.bytes_len = bytes_len; a.off = off; a.bias = bias; a.n = n; a.out = out;
    a.hdr = hdr; a.direct = e->keys_direct ? 1u : 0u;
    HIP_OK(launch_hash_keys(a, e->stream));
    return RL_OK;
}

extern "C" int rl_hash_keys_device(rl_engine* e, size_t n, const uint8_t* key_bytes, size_t key_bytes_len,
                                   const uint64_t* key_off, uint64_t* key_hash, uint64_t* hdr,
                                   void* stream) {
    if (!e) return RL_E_INVALID_ARG;
    if ((n && (!key_off || !key_hash)) || !hdr || (key_bytes_len && !key_bytes)) return RL_E_INVALID_ARG;
    if (((uintptr_t)key_off | (uintptr_t)key_hash | (uintptr_t)hdr) & 7u) return RL_E_INVALID_ARG;
    if ((uint64_t)n > kKeysMaxN) return RL_E_TOO_LARGE;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    StreamJoin join(e->stream, (hipStream_t)stream);
    HIP_OK(join.err);
    const int rc = hash_keys_enqueue(e, n, key_bytes, key_bytes_len, key_off, 0, key_hash,
                                     (unsigned long long*)hdr);
    HIP_OK(join.finish());
    return rc;
}

// The arguments of the two host forms; every offset is checked before any device call.
static bool keys_host_args_ok(size_t n, const uint8_t* key_bytes, size_t key_bytes_len, const uint64_t* key_off) {
    if (n == 0) return true;
    if (!key_off || (key_bytes_len && !key_bytes) || ((uintptr_t)key_off & 7u)) return false;
    return keys_first_malformed(key_off, n, key_bytes_len) == n;
}

// The blob stage and room for `keys` offsets (+ 1) and hashes.
static int ensure_key_stage(rl_engine* e, size_t keys) {
    if (e->ks_blob_cap != e->key_stage_bytes) {
        dfree(e->ks_blob);
        e->ks_blob_cap = 0;
        int rc = dalloc(&e->ks_blob, e->key_stage_bytes);
        if (rc != RL_OK) return rc;
        e->ks_blob_cap = e->key_stage_bytes;
    }
    if (!e->ks_hdr) {
        int rc = dalloc(&e->ks_hdr, 2);
        if (rc != RL_OK) return rc;
    }
    if (keys > e->ks_keys_cap) {
        dfree(e->ks_off); dfree(e->ks_hash);
        e->ks_keys_cap = 0;
        int rc = dalloc(&e->ks_off, keys + 1);
        if (rc == RL_OK) rc = dalloc(&e->ks_hash, keys);
        if (rc != RL_OK) return rc;
        e->ks_keys_cap = keys;
    }
    return RL_OK;
}

// One staged chunk: keys [at, at + m) of the host batch hashed into out[0, m) (device). The
// chunk's bytes go through ks_blob; `d_off` holds the chunk's m + 1 offsets on the device.
static int hash_keys_chunk(rl_engine* e, const uint8_t* key_bytes, const uint64_t* key_off, size_t at,
                           size_t m, const uint64_t* d_off, uint64_t* out) {
    const uint64_t base = key_off[at], bytes = key_off[at + m] - base;
    if (bytes) HIP_OK(hipMemcpyAsync(e->ks_blob, key_bytes + base, bytes, hipMemcpyHostToDevice, e->stream));
    return hash_keys_enqueue(e, m, e->ks_blob, bytes, d_off, base, out, e->ks_hdr);
}

extern "C" int rl_hash_keys(rl_engine* e, size_t n, const uint8_t* key_bytes, size_t key_bytes_len,
                            const uint64_t* key_off, uint64_t* key_hash) {
    if (!e) return RL_E_INVALID_ARG;
    if ((n && !key_hash) || !keys_host_args_ok(n, key_bytes, key_bytes_len, key_off)) return RL_E_INVALID_ARG;
    if (n == 0) return RL_OK;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    const size_t max_keys = (size_t)std::min<uint64_t>(e->opts.max_batch, n);
    int rc = ensure_key_stage(e, max_keys);
    if (rc != RL_OK) return rc;
    hipStream_t s = e->stream;
    for (size_t at = 0; at < n;) {
        const size_t m = keys_chunk(key_off, n, at, max_keys, e->key_stage_bytes);
        HIP_OK(hipMemcpyAsync(e->ks_off, key_off + at, (m + 1) * 8, hipMemcpyHostToDevice, s));
        rc = hash_keys_chunk(e, key_bytes, key_off, at, m, e->ks_off, e->ks_hash);
        if (rc != RL_OK) { (void)hipStreamSynchronize(s); return rc; }
        HIP_OK(hipMemcpyAsync(key_hash + at, e->ks_hash, m * 8, hipMemcpyDeviceToHost, s));
        at += m;
    }
    HIP_OK(hipStreamSynchronize(s));
    return RL_OK;
}

extern "C" int rl_execute_batch_keys(rl_engine* e, size_t n, const uint8_t* key_bytes, size_t key_bytes_len,
                                     const uint64_t* key_off, const int32_t* permits, const int64_t* now_ns,
                                     const uint16_t* limiter, const uint8_t* op, uint8_t* allowed,
                                     int64_t* remaining, double* tokens_after, uint64_t* key_hash_out) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (n > e->opts.max_batch) return RL_E_TOO_LARGE;
    if (n == 0) return RL_OK;
    if (!permits || !now_ns || !allowed || !remaining) return RL_E_INVALID_ARG;
    if (!keys_host_args_ok(n, key_bytes, key_bytes_len, key_off)) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    int rc = ensure_key_stage(e, n);
    if (rc == RL_OK) rc = stage_requests(e, n, nullptr, permits, now_ns, limiter, op);
    if (rc != RL_OK) return rc;
    hipStream_t s = e->stream;
    HIP_OK(hipMemcpyAsync(e->ks_off, key_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    for (size_t at = 0; at < n;) {                     // byte chunks, hashed straight into s_key
        const size_t m = keys_chunk(key_off, n, at, n, e->key_stage_bytes);
        rc = hash_keys_chunk(e, key_bytes, key_off, at, m, e->ks_off + at, e->s_key + at);
        if (rc != RL_OK) { (void)hipStreamSynchronize(s); return rc; }
        at += m;
    }
    if (key_hash_out) HIP_OK(hipMemcpyAsync(key_hash_out, e->s_key, n * 8, hipMemcpyDeviceToHost, s));
    return run_staged_batch(e, n, limiter != nullptr, op != nullptr, allowed, remaining, tokens_after);
}

// ---------------------------------------------------------------- table digest
// rl_digest.hip on the engine stream, under the census' rules (above): behind every batch
// submitted before, the table as installed, no collect_status, nothing written but `out`.
static_assert(RL_DIGEST_K_SW == kDigestKSw && RL_DIGEST_K_TB == kDigestKTb &&
              RL_DIGEST_K_CACHE == kDigestKCache && RL_DIGEST_C1 == kDigestC1 &&
              RL_DIGEST_C2 == kDigestC2, "digest constants");
static_assert(sizeof(rl_bucket_digest) == 24 && sizeof(BucketDigest) == 24, "rl_bucket_digest layout");

static bool digest_args_ok(const rl_engine* e, size_t limiter, uint32_t bucket_bits, uint32_t flags) {
    if (limiter >= e->lims.size() || (flags & ~(uint32_t)RL_DIGEST_CACHE)) return false;
    return bucket_bits <= (uint32_t)e->lims[limiter].dev.region_bits;
}

// Zeroes out[2^bucket_bits] (device) and launches the pass, both on the engine stream; for few
// buckets the pass writes finer ones into e->digest_fine and a fold fills `out` (rl_digest.hip).
static int digest_enqueue(rl_engine* e, size_t li, int64_t now_ns, uint32_t bucket_bits, uint32_t flags,
                          BucketDigest* out) {
    const HostLimiter& h = e->lims[li];
    DigestArgs a{};
    a.tab = (const Slot*)h.table;
    a.n_regions = h.table_bytes / sizeof(Slot) / kRegionSlots;
    a.L = h.dev;
    a.now = floor_div_ms(now_ns);
    a.bucket_bits = bucket_bits;
    a.with_cache = (flags & RL_DIGEST_CACHE) ? 1u : 0u;
    a.out = out;
    a.per_cu = e->digest_per_cu;
    if (a.n_regions != (1ULL << h.dev.region_bits)) return RL_E_INTERNAL;   // (buckets are region ranges)
    const uint32_t fine = std::min<uint32_t>(kDigestFineBits, (uint32_t)h.dev.region_bits);
    if (bucket_bits < fine) {
        if (!e->digest_fine) {
            int rc = dalloc(&e->digest_fine, (size_t)1 << kDigestFineBits);
            if (rc != RL_OK) return rc;
        }
        a.bucket_bits = fine;
        a.out = e->digest_fine;
    }
    HIP_OK(hipMemsetAsync(a.out, 0, sizeof(BucketDigest) << a.bucket_bits, e->stream));
    HIP_OK(launch_digest(a, e->stream));
    if (a.out != out) HIP_OK(launch_digest_fold(a.out, fine, out, bucket_bits, e->stream));
    return RL_OK;
}

extern "C" int rl_limiter_digest_device(rl_engine* e, uint16_t limiter, int64_t now_ns,
                                        uint32_t bucket_bits, uint32_t flags, rl_bucket_digest* out,
                                        void* stream) {
    if (!e || !out || ((uintptr_t)out & 7u)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!digest_args_ok(e, limiter, bucket_bits, flags)) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    StreamJoin join(e->stream, (hipStream_t)stream);
    HIP_OK(join.err);
    int rc = digest_enqueue(e, limiter, now_ns, bucket_bits, flags, (BucketDigest*)out);
    if (rc != RL_OK) return rc;
    HIP_OK(join.finish());
    return RL_OK;
}

extern "C" int rl_limiter_digest(rl_engine* e, uint16_t limiter, int64_t now_ns, uint32_t bucket_bits,
                                 uint32_t flags, rl_bucket_digest* out, rl_bucket_digest* total) {
    if (!e || !out) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (!digest_args_ok(e, limiter, bucket_bits, flags)) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    const size_t nb = (size_t)1 << bucket_bits;
    if (nb > e->digest_cap) {                         // (freeing waits for the device)
        dfree(e->digest);
        e->digest_cap = 0;
        int rc = dalloc(&e->digest, nb);
        if (rc != RL_OK) return rc;
        e->digest_cap = nb;
    }
    int rc = digest_enqueue(e, limiter, now_ns, bucket_bits, flags, e->digest);
    if (rc != RL_OK) return rc;
    HIP_OK(hipMemcpyAsync(out, e->digest, nb * sizeof(BucketDigest), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (total) {
        rl_bucket_digest t{0, 0, 0};
        for (size_t b = 0; b < nb; ++b) {
            t.entries += out[b].entries; t.sum += out[b].sum; t.xr ^= out[b].xr;
        }
        *total = t;
    }
    return RL_OK;
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
    if (std::strcmp(key, "ablate") == 0) { e->ablate = (uint32_t)value; return RL_OK; }
    if (std::strcmp(key, "upsweep_per_cu") == 0) { e->up_per_cu = (uint32_t)value; return RL_OK; }
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
        e->hot_threshold = (uint32_t)value;
        e->hot_thr_auto = false;
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
        e->route = value != 0;
        return RL_OK;
    }
    if (std::strcmp(key, "tile_items") == 0) {        // partition tile = value x 512 requests
        if (value != 0 && (value < 8 || value > 1024 || value % 8 != 0)) return RL_E_INVALID_ARG;
        e->tile_items = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "segments") == 0) {          // two-pass batches: pass-0 output segments
        if (value < 1 || value > 64) return RL_E_INVALID_ARG;
        e->segments = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "group_bits") == 0) {        // two-pass batches: pass-0 high-digit bits
        if (value < 1 || value > kMaxDigitBits) return RL_E_INVALID_ARG;
        e->group_bits = (uint32_t)value;
        return RL_OK;
    }
    if (std::strcmp(key, "walk") == 0) {              // allow walks of the hot chains
        e->walk = value != 0;
        if (!e->walk && e->walk_tab) {                 // (hipFree waits for the batches in flight)
            HIP_OK(hipStreamSynchronize(e->stream));
            if (e->hstream) HIP_OK(hipStreamSynchronize(e->hstream));
            dfree(e->walk_tab);
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
    if (e->pending_status) {                                 // the last batch is complete
        e->hot_hint = e->h_ctl->n_hot;
        e->walk_hint = e->h_ctl->n_walk;
    }
    return RL_OK;
}

extern "C" int rl_route_partition(rl_engine* e, size_t n, const uint64_t* key_hash,
                                  const uint16_t*, uint32_t shard_count, uint32_t* perm,
                                  uint64_t* counts_host, void* stream) {
    if (!e || !key_hash || !perm || !counts_host) return RL_E_INVALID_ARG;
    if (shard_count == 0 || shard_count > 64 || (shard_count & (shard_count - 1))) return RL_E_INVALID_ARG;
    if (n > 0xFFFFFFF0ULL) return RL_E_TOO_LARGE;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    const size_t nt = (n + kTile - 1) / kTile;
    const size_t need = (size_t)shard_count * nt + 64;
    if (need > e->route_cap) {
        dfree(e->route_scratch);
        if (dalloc(&e->route_scratch, need) != RL_OK) return RL_E_NOMEM;
        e->route_cap = need;
    }
    if (!e->route_counts && dalloc(&e->route_counts, 64) != RL_OK) return RL_E_NOMEM;
    if (n == 0) {
        for (uint32_t i = 0; i < shard_count; ++i) counts_host[i] = 0;
        return RL_OK;
    }
    HIP_OK(launch_owner_partition(key_hash, (uint32_t)n, shard_count, perm, e->route_counts,
                                  e->route_scratch, e->d_dir, s));
    uint32_t c[64];
    HIP_OK(hipMemcpyAsync(c, e->route_counts, shard_count * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < shard_count; ++i) counts_host[i] = c[i];
    return RL_OK;
}

// Hot-key owner directory: key_hash[i] is owned by owner[i] instead of its hash owner.
// Every rank of a router must install the same directory, before any state exists for
// those keys. That holds for this call and rl_router_plan_directory only:
// rl_router_replan_directory moves the state of the keys that change owner (rl_copy_keys /
// rl_put_keys / rl_drop_keys below) and then installs the directory through this call.
extern "C" int rl_set_owner_directory(rl_engine* e, size_t n, const uint64_t* key_hash,
                                      const uint32_t* owner) {
    if (!e || (n && (!key_hash || !owner)) || n > kDirMax) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    for (size_t i = 0; i < n; ++i)
        if (owner[i] >= e->opts.shard_count) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    if (n == 0) {
        dfree(e->d_dir);
        e->h_dir.clear();
        return RL_OK;
    }
    std::vector<DirSlot> t(kDirSlots, DirSlot{0, kDirEmpty, 0});
    for (size_t i = 0; i < n; ++i) {
        const uint64_t tag = mix64(key_hash[i]);
        uint32_t p = (uint32_t)tag & (kDirSlots - 1);
        while (t[p].owner != kDirEmpty && t[p].tag != tag) p = (p + 1) & (kDirSlots - 1);
        t[p].tag = tag;
        t[p].owner = owner[i];
    }
    if (!e->d_dir && dalloc(&e->d_dir, kDirSlots) != RL_OK) return RL_E_NOMEM;
    HIP_OK(hipMemcpy(e->d_dir, t.data(), kDirSlots * sizeof(DirSlot), hipMemcpyHostToDevice));
    e->h_dir.swap(t);
    return RL_OK;
}

extern "C" uint32_t rl_owner_of_engine(rl_engine* e, uint64_t key_hash) {
    if (!e) return 0;
    const uint64_t tag = mix64(key_hash);
    if (!e->h_dir.empty()) {
        uint32_t p = (uint32_t)tag & (kDirSlots - 1);
        for (uint32_t i = 0; i < kDirSlots && e->h_dir[p].owner != kDirEmpty; ++i) {
            if (e->h_dir[p].tag == tag) return e->h_dir[p].owner;
            p = (p + 1) & (kDirSlots - 1);
        }
    }
    return e->opts.shard_count <= 1 ? 0u : (uint32_t)(tag >> (64 - e->shard_bits));
}

extern "C" int rl_route_pack(rl_engine* e, size_t n, const uint32_t* perm, const uint64_t* key,
                             const int32_t* permits, const int64_t* now_ns, const uint16_t* limiter,
                             uint64_t* key_out, int32_t* permits_out, int64_t* now_out,
                             uint16_t* limiter_out, void* stream) {
    if (!e || (n && (!perm || !key || !permits || !now_ns || !key_out || !permits_out || !now_out)))
        return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_pack((uint32_t)n, perm, key, permits, now_ns, limiter, key_out, permits_out,
                             now_out, limiter_out, s));
    return RL_OK;
}

extern "C" int rl_route_fold(rl_engine* e, size_t n, const uint8_t* allowed, const int64_t* remaining,
                             int64_t* packed, void* stream) {
    if (!e || (n && (!allowed || !remaining || !packed))) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_fold((uint32_t)n, allowed, remaining, packed, s));
    return RL_OK;
}

extern "C" int rl_route_unpack(rl_engine* e, size_t n, const uint32_t* perm, const int64_t* packed,
                               uint8_t* allowed, int64_t* remaining, void* stream) {
    if (!e || (n && (!perm || !packed || !allowed || !remaining))) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_unpack((uint32_t)n, perm, packed, allowed, remaining, s));
    return RL_OK;
}

extern "C" int rl_route_pack_wire(rl_engine* e, size_t n, const uint32_t* perm, const uint64_t* key,
                                  const int32_t* permits, const int64_t* now_ns,
                                  const uint16_t* limiter, uint64_t* wire_out,
                                  uint16_t* limiter_out, int64_t* hdr, void* stream) {
    if (!e || !hdr || (n && (!perm || !key || !permits || !now_ns || !wire_out))) return RL_E_INVALID_ARG;
    if (n > 0xFFFFFFF0ULL) return RL_E_TOO_LARGE;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_pack_wire((uint32_t)n, perm, key, permits, now_ns, limiter, wire_out,
                                  limiter_out, hdr, s));
    return RL_OK;
}

namespace rl {
// rl_route_pack_wire plus the per-block now_ms min / max partials of the router's header
// (internal: rl_router.cpp).
int route_pack_wire_mm(rl_engine* e, size_t n, const uint32_t* perm, const uint64_t* key,
                       const int32_t* permits, const int64_t* now_ns, const uint16_t* limiter,
                       uint64_t* wire_out, uint16_t* limiter_out, int64_t* hdr, uint64_t* part,
                       uint32_t* nparts, void* stream, const int64_t* live_counts,
                       uint32_t live_stride, uint32_t live_g) {
    if (!e || !hdr || !part || !nparts || (n && (!perm || !key || !permits || !now_ns || !wire_out)))
        return RL_E_INVALID_ARG;
    if (n > 0xFFFFFFF0ULL) return RL_E_TOO_LARGE;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_pack_wire((uint32_t)n, perm, key, permits, now_ns, limiter, wire_out,
                                  limiter_out, hdr, s, part, nparts, live_counts, live_stride, live_g));
    return RL_OK;
}
int engine_device(rl_engine* e) { return e ? e->device : 0; }
size_t engine_max_batch(rl_engine* e) { return e ? (size_t)e->opts.max_batch : 0; }
size_t engine_limiters(rl_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return e->lims.size();
}
size_t engine_directory(rl_engine* e, uint64_t* keys, uint32_t* owners) {
    if (!e || !keys || !owners) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    size_t n = 0;
    for (const DirSlot& d : e->h_dir)
        if (d.owner != kDirEmpty && n < kDirMax) { keys[n] = unmix64(d.tag); owners[n++] = d.owner; }
    return n;
}
}  // namespace rl

extern "C" int rl_route_unwire(rl_engine* e, size_t m, const uint64_t* wire, uint32_t n_src,
                               const int64_t* src_base, const uint64_t* src_count,
                               uint64_t* key_out, int32_t* permits_out, int64_t* now_out,
                               void* stream) {
    if (!e || !src_base || !src_count || n_src == 0 || n_src > (uint32_t)kMaxShards)
        return RL_E_INVALID_ARG;
    if (m && (!wire || !key_out || !permits_out || !now_out)) return RL_E_INVALID_ARG;
    if (m > 0xFFFFFFF0ULL) return RL_E_TOO_LARGE;
    uint32_t end[kMaxShards];
    uint64_t run = 0;
    for (uint32_t i = 0; i < n_src; ++i) { run += src_count[i]; end[i] = (uint32_t)run; }
    if (run != m) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_unwire((uint32_t)m, wire, n_src, src_base, end, key_out, permits_out,
                               now_out, s));
    return RL_OK;
}

extern "C" int rl_result_width(rl_engine* e) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    bool wide = false;
    int64_t max_any = 0;
    for (auto& l : e->lims) {
        wide |= l.cfg.max_permits > kCompactMaxPermits;
        max_any = std::max<int64_t>(max_any, l.cfg.max_permits);
    }
    return res_bytes_for(max_any, wide);
}

extern "C" int rl_route_fold_packed(rl_engine* e, size_t n, const uint8_t* allowed,
                                    const int64_t* remaining, void* packed, int width,
                                    void* stream) {
    if (!e || (n && (!allowed || !remaining || !packed))) return RL_E_INVALID_ARG;
    if (width != 1 && width != 2 && width != 4 && width != 8) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_fold_w((uint32_t)n, allowed, remaining, packed, width, s));
    return RL_OK;
}

extern "C" int rl_route_unpack_packed(rl_engine* e, size_t n, const uint32_t* perm,
                                      const void* packed, int width, uint8_t* allowed,
                                      int64_t* remaining, void* stream) {
    if (!e || (n && (!perm || !packed || !allowed || !remaining))) return RL_E_INVALID_ARG;
    if (width != 1 && width != 2 && width != 4 && width != 8) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_unpack_w((uint32_t)n, perm, packed, width, allowed, remaining, s));
    return RL_OK;
}

extern "C" uint64_t rl_route_return_bytes(uint32_t n_seg, const uint64_t* seg_counts, int width,
                                          uint32_t exc_cap) {
    if (!seg_counts || n_seg == 0 || n_seg > (uint32_t)kMaxShards) return 0;
    if (width != 1 && width != 2 && width != 4 && width != 8) return 0;
    return ret_layout(seg_counts, n_seg, width, exc_cap, nullptr, nullptr);
}

extern "C" int rl_route_fold_return(rl_engine* e, size_t m, const uint8_t* allowed,
                                    const int64_t* remaining, void* out, int width, uint32_t n_seg,
                                    const uint64_t* seg_counts, uint32_t exc_cap, void* stream) {
    if (!e || !out || !seg_counts || (m && (!allowed || !remaining))) return RL_E_INVALID_ARG;
    if (width != 1 && width != 2 && width != 4 && width != 8) return RL_E_INVALID_ARG;
    if (n_seg == 0 || n_seg > (uint32_t)kMaxShards || m > 0xFFFFFFF0ULL) return RL_E_INVALID_ARG;
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n_seg; ++i) tot += seg_counts[i];
    if (tot != m) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_fold_ret((uint32_t)m, allowed, remaining, out, width, n_seg, seg_counts,
                                 exc_cap, s));
    return RL_OK;
}

extern "C" int rl_route_unpack_return(rl_engine* e, size_t n, const uint32_t* perm, const void* in,
                                      int width, uint32_t n_seg, const uint64_t* seg_counts,
                                      uint32_t exc_cap, uint8_t* allowed, int64_t* remaining,
                                      uint32_t* lost, void* stream) {
    if (!e || !seg_counts || !lost || (n && (!perm || !in || !allowed || !remaining)))
        return RL_E_INVALID_ARG;
    if (width != 1 && width != 2 && width != 4 && width != 8) return RL_E_INVALID_ARG;
    if (n_seg == 0 || n_seg > (uint32_t)kMaxShards || n > 0xFFFFFFF0ULL) return RL_E_INVALID_ARG;
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n_seg; ++i) tot += seg_counts[i];
    if (tot != n) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_unpack_ret((uint32_t)n, perm, in, width, n_seg, seg_counts, exc_cap, allowed,
                                   remaining, lost, s));
    return RL_OK;
}

extern "C" int rl_route_partition_device(rl_engine* e, size_t n, const uint64_t* key_hash,
                                         uint32_t shard_count, uint32_t* perm, int64_t* counts_dev,
                                         size_t counts_stride, void* stream) {
    if (!e || !key_hash) return RL_E_INVALID_ARG;
    return rl_route_partition_skip_device(e, n, key_hash, nullptr, shard_count, perm, counts_dev,
                                          counts_stride, stream);
}

extern "C" int rl_route_fold_ops(rl_engine* e, size_t n, const uint32_t* perm, const uint16_t* limiter,
                                 const uint8_t* op, uint16_t* col, void* stream) {
    if (!e || (n && (!perm || !col))) return RL_E_INVALID_ARG;
    if (n > 0xFFFFFFF0ULL) return RL_E_TOO_LARGE;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_fold_ops((uint32_t)n, perm, limiter, op, col, s));
    return RL_OK;
}

extern "C" int rl_route_unfold_ops(rl_engine* e, size_t m, const uint16_t* col, uint16_t* limiter_out,
                                   uint8_t* op_out, void* stream) {
    if (!e || (m && (!col || !limiter_out || !op_out))) return RL_E_INVALID_ARG;
    if (m > 0xFFFFFFF0ULL) return RL_E_TOO_LARGE;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_unfold_ops((uint32_t)m, col, limiter_out, op_out, s));
    return RL_OK;
}

extern "C" int rl_route_unpack_wait(rl_engine* e, size_t n, size_t n_live, const uint32_t* perm,
                                    const int64_t* back, const uint8_t* skip, int64_t* wait_ms,
                                    void* stream) {
    if (!e || n_live > n || (n && !wait_ms) || (n_live && (!perm || !back))) return RL_E_INVALID_ARG;
    if (n > 0xFFFFFFF0ULL) return RL_E_TOO_LARGE;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_route_unpack_wait((uint32_t)n, (uint32_t)n_live, perm, back, skip, wait_ms, s));
    return RL_OK;
}

extern "C" int rl_route_partition_skip_device(rl_engine* e, size_t n, const uint64_t* key_hash,
                                              const uint8_t* skip, uint32_t shard_count,
                                              uint32_t* perm, int64_t* counts_dev,
                                              size_t counts_stride, void* stream) {
    if (!e || (n && !key_hash) || !perm || !counts_dev || counts_stride == 0) return RL_E_INVALID_ARG;
    if (shard_count == 0 || shard_count > 64 || (shard_count & (shard_count - 1))) return RL_E_INVALID_ARG;
    if (n > 0xFFFFFFF0ULL) return RL_E_TOO_LARGE;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    const size_t nt = (n + kTile - 1) / kTile;
    const size_t need = (size_t)shard_count * std::max<size_t>(nt, 1) + 64;
    if (need > e->route_cap) {
        dfree(e->route_scratch);
        if (dalloc(&e->route_scratch, need) != RL_OK) return RL_E_NOMEM;
        e->route_cap = need;
    }
    if (!e->route_counts && dalloc(&e->route_counts, 64) != RL_OK) return RL_E_NOMEM;
    if (n == 0) {
        HIP_OK(hipMemsetAsync(e->route_counts, 0, 64 * sizeof(uint32_t), s));
    } else {
        HIP_OK(launch_owner_partition(key_hash, (uint32_t)n, shard_count, perm, e->route_counts,
                                      e->route_scratch, e->d_dir, s, skip));
    }
    HIP_OK(launch_counts_to_header(e->route_counts, shard_count, counts_dev, (uint32_t)counts_stride, s));
    return RL_OK;
}

extern "C" int rl_synth_trace_device(rl_engine* e, const rl_trace_spec* sp, size_t n,
                                     uint64_t* key_hash, int32_t* permits, int64_t* now_ns,
                                     uint16_t* limiter, void* stream) {
    if (!e || !sp || !key_hash || !permits || !now_ns) return RL_E_INVALID_ARG;
    if (sp->n_keys == 0 || sp->permits_max <= 0 || sp->n_total == 0) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    SynthArgs a{};
    a.seed = sp->seed; a.n_keys = sp->n_keys; a.dist = sp->dist; a.permits_max = sp->permits_max;
    a.t0_ns = sp->t0_ns; a.span_ns = sp->span_ns; a.index_base = sp->index_base;
    a.n_total = sp->n_total; a.n_limiters = sp->n_limiters ? sp->n_limiters : 1;
    a.key = key_hash; a.permits = permits; a.now_ns = now_ns; a.limiter = limiter; a.n = n;
    if (sp->dist == RL_DIST_ZIPF) {
        const double s = sp->zipf_s;
        if (!(s > 0.0) || s == 1.0) return RL_E_INVALID_ARG;
        auto h1 = [](double x) { return std::fabs(x) > 1e-8 ? std::log1p(x) / x : 1.0 - x * (0.5 - x / 3.0); };
        auto h2 = [](double x) { return std::fabs(x) > 1e-8 ? std::expm1(x) / x : 1.0 + x * 0.5 * (1.0 + x / 3.0); };
        auto H = [&](double x) { double lx = std::log(x); return h2((1.0 - s) * lx) * lx; };
        auto hh = [&](double x) { return std::exp(-s * std::log(x)); };
        auto Hinv = [&](double x) { double t = x * (1.0 - s); if (t < -1.0) t = -1.0; return std::exp(h1(t) * x); };
        a.zs = s;
        a.hx1 = H(1.5) - 1.0;
        a.hn = H((double)sp->n_keys + 0.5);
        a.sconst = 2.0 - Hinv(H(2.5) - hh(2.0));
    }
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    HIP_OK(launch_synth(a, st));
    return RL_OK;
}

extern "C" int rl_debug_fetch(rl_engine* e, const char* what, void* out, size_t bytes) {
    if (!e || !what || (!out && bytes)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (std::strcmp(what, "region_times") == 0) {
        if (!e->dbg) return RL_E_INVALID_ARG;
        HIP_OK(hipStreamSynchronize(e->stream));
        const size_t nb = std::min(bytes, e->dbg_cap * sizeof(uint64_t));
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
    DevBuf<StateRec> d_out;
    DevBuf<uint32_t> d_count;
    if (d_out.alloc(std::max<uint32_t>(dcap, 1u)) != RL_OK || d_count.alloc(1) != RL_OK) return RL_E_NOMEM;
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
    DevBuf<uint8_t> d;
    if (d.alloc(bytes) != RL_OK) return RL_E_NOMEM;
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
    DevBuf<uint64_t> d_keys;
    DevBuf<KeyImage> d_out;
    DevBuf<uint32_t> d_count;
    if (d_keys.alloc(nk) != RL_OK || d_out.alloc(std::max<uint32_t>(dcap, 1u)) != RL_OK ||
        d_count.alloc(1) != RL_OK)
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
    if (!e->snap) {
        int rc = dalloc(&e->snap, snap_scratch_bytes());
        if (rc != RL_OK) return rc;
    }
    *sc = snap_scratch_at(e->snap);
    return RL_OK;
}

// (growing either buffer frees the old one, which waits for the device: nothing still reads it)
static int ensure_put_heads(rl_engine* e, size_t n) {
    if (n <= e->put_heads_cap) return RL_OK;
    dfree(e->put_heads);
    e->put_heads_cap = 0;
    int rc = dalloc(&e->put_heads, n);
    if (rc == RL_OK) e->put_heads_cap = n;
    return rc;
}

static int ensure_img_stage(rl_engine* e, size_t n) {
    if (n <= e->img_stage_cap) return RL_OK;
    dfree(e->img_stage);
    e->img_stage_cap = 0;
    int rc = dalloc(&e->img_stage, n);
    if (rc == RL_OK) e->img_stage_cap = n;
    return rc;
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
    rc = ensure_img_stage(e, (size_t)std::min<uint64_t>(cap, m * kRegionSlots));
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
    if (rc == RL_OK) rc = ensure_put_heads(e, n);
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
    if (rc == RL_OK) rc = ensure_put_heads(e, piece);
    if (rc == RL_OK) rc = ensure_img_stage(e, piece);
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
    DevBuf<uint32_t> d_count;
    if (d_count.alloc(h.size()) != RL_OK) return RL_E_NOMEM;
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
    DevBuf<unsigned char> buf;
    if (buf.alloc(shrink_scratch_bytes(n_regions)) != RL_OK) return RL_E_NOMEM;
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
    DevBuf<uint32_t> fail;
    auto drop = [&] { for (Tab& t : tabs) { dfree(t.t); dfree(t.x); } };
    int rc = fail.alloc(1);
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
