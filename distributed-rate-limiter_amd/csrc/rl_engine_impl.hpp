// rl_engine_impl.hpp — what the units of the host runtime share (rl_engine*.cpp): the engine
// struct, the owning device-buffer type and the few helpers that cross units. Private to them.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/rl_engine.h"
#include "rl_launch.hpp"

// nothing from here on is part of the library's interface (the plan's inline functions included)
#pragma GCC visibility push(hidden)
#include "rl_batch_plan.hpp"

#define HIP_OK(x)                                                     \
    do {                                                               \
        hipError_t _e = (x);                                           \
        if (_e != hipSuccess) {                                        \
            std::fprintf(stderr, "rl_engine: %s failed: %s (%s:%d)\n", #x, \
                         hipGetErrorString(_e), __FILE__, __LINE__);   \
            return RL_E_DEVICE;                                        \
        }                                                              \
    } while (0)

// Raw device memory: the limiter tables only (HostLimiter); everything else is a DevArray.
inline void dfree(void*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}
inline int dalloc(void** p, size_t bytes) {
    if (rl::dev_malloc(p, bytes ? bytes : 16) != hipSuccess) {
        *p = nullptr;
        return RL_E_NOMEM;
    }
    return RL_OK;
}

// A device buffer of `cap` elements, freed with its owner. reserve() never keeps the contents
// and adds no headroom: where a buffer grows with slack, the caller passes the larger count.
template <class T>
struct DevArray {
    T* p = nullptr;
    size_t cap = 0;
    DevArray() = default;
    DevArray(const DevArray&) = delete;
    DevArray& operator=(const DevArray&) = delete;
    ~DevArray() { free(); }
    void free() {
        if (p) (void)hipFree((void*)p);
        p = nullptr;
        cap = 0;
    }
    // (freeing waits for the device: nothing still uses the old buffer afterwards)
    int reserve(size_t count) {
        if (count <= cap) return RL_OK;
        free();
        if (dalloc((void**)&p, count * sizeof(T)) != RL_OK) return RL_E_NOMEM;
        cap = count;
        return RL_OK;
    }
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

// Stage timing: events bracket every kernel of a batch; a ring of per-batch event
// sets is averaged when rl_stage_times is called (no host sync inside a batch).
constexpr int kMarks = 12;   // marks 0..11 on the engine stream
constexpr int kEvRing = 64;

// The tables are raw pointers with explicit frees: grow_once and shrink_by swap them with
// rollback, and the record is copied into rl_engine::lims.
struct HostLimiter {
    rl_limiter_config cfg;
    rl::DevLimiter dev;
    void* table = nullptr;
    size_t table_bytes = 0;
    void* cache_table = nullptr;            // SW local cache: u64 per slot
};

// Per-batch scratch: the partition's records/positions, the [bin][tile] counts, the packed
// results and the batch control block. Two sets, so that with RL_OPT_PIPELINE the partition
// of batch k+1 (its own stream) can run while batch k's region stage still reads its set.
struct BatchScratch {
    size_t cap_n = 0;                       // requests the arrays up to `tok` hold (ensure_scratch)
    bool cap_wide = false;
    DevArray<uint8_t> rec0, rec1;           // records (RecC or RecW)
    DevArray<uint32_t> pos0, pos1;
    DevArray<uint16_t> digit;               // routing: pass-0 digit per request
    DevArray<uint64_t> res;
    DevArray<int64_t> ext;                  // escaped remainders (kResEscape), like res
    DevArray<double> tok;
    DevArray<uint32_t> counts;              // [bins][tiles]
    DevArray<uint32_t> bin_total;           // [2^kMaxDigitBits]
    DevArray<uint32_t> bin_base;            // [2^kMaxDigitBits]
    DevArray<uint32_t> region_count;        // [P padded]
    DevArray<uint32_t> region_start;
    DevArray<uint32_t> gtile;               // k_group*: tile_base, tile_bin, per-tile counts
    DevArray<uint32_t> seg;                 // segmented pass 0: seg_adj, seg_start, seg_cnt
    DevArray<rl::BatchCtl> d_ctl;
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
    DevArray<rl::DevLimiter> d_lims;
    DevArray<uint8_t> d_region_lim;

    // per-batch scratch (sized for opts.max_batch); sc[0] unless pipelined
    BatchScratch sc[2];
    int next_set = 0;
    bool pipeline = false;                  // RL_OPT_PIPELINE
    hipStream_t pstream = nullptr;          // partition stream (pipeline)
    hipEvent_t in_ev = nullptr;             // pipeline: inputs ready on e->stream
    hipStream_t hstream = nullptr;          // hot chains beside the normal regions
    hipEvent_t hot_ev[2] = {};              // fork, join of hstream
    // hot regions
    DevArray<uint32_t> hot_list;            // [kHotListWords]: list, k_hot_select's meta, totals
    DevArray<rl::HotInfo> hot_info;         // [kHotMax]
    DevArray<uint64_t> hot_summ;            // [need][8] (ensure_hot_summ)
    size_t hot_summ_l1 = 0;
    DevArray<uint2> walk_tab;               // [kWalkTabEntries] allow-walk tables (hot chains)
    bool walk = true;                       // rl_tune("walk"): allow walks in the hot chains
    uint32_t walk_hint = 0;                 // listed regions that wanted a walk in the last batch
                                            // seen complete (walk_tab is allocated once it is > 0)
    uint32_t walk_min = rl::kWalkMinAllows; // rl_tune("walk_min"): fewest expected allows walked
    bool chain_split = true;                // rl_tune("chain_split"): two-wave hot chains
    DevArray<uint32_t> hot_mark;            // epoch marks per bin
    uint32_t epoch = 0;
    // rl_tune: tile_items, segments, group_bits, hot_threshold (auto until set), route,
    // upsweep_per_cu. Hot-region routing (two-pass batches): the previous batch's hot regions get
    // pass-0 bins of their own and skip pass 1. route_list holds region ids (kNone = unused); it
    // is built on device at the end of each batch's hot preparation and cleared when region ids
    // change.
    rl::BatchTune tune;
    bool region_order = true;               // rl_tune("region_order"): largest regions dispatched first
    uint32_t order_prefix = 4096;           // rl_tune("order_prefix"): ... after this many of the smallest
    DevArray<uint32_t> order;               // [regions + 1]
    DevArray<uint32_t> order_meta;          // [kOrderMeta]
    // One table per scratch set: with RL_OPT_PIPELINE batch k+1's partition runs while batch
    // k's region stage still reads its routed ranges and writes the next table, so batch k uses
    // set k % 2's table, written by batch k - 2 (set 0 only without the option: batch k - 1).
    DevArray<uint32_t> route_list;          // [2][kRouteWords] region ids (kNone = empty), dense indices
    DevArray<uint32_t> route_start;         // [2][kRouteSlots] this batch's routed bins
    DevArray<uint32_t> route_cnt;           // [2][kRouteSlots]
    uint32_t solo_threshold = 4096;         // rl_tune("solo_threshold"): records per cache-on SW
                                            // region for the single-key allow-run pass (0: off)
    DevArray<uint32_t> solo_list;           // [kSoloMax + 1]: the listed regions, then their count
    uint32_t sparse_max = 96;               // rl_tune("sparse_max"): records per region up to
                                            // which a region probes single buckets; 0 = never
    DevArray<uint64_t> dbg;                 // rl_tune("debug_regions"): per-bin stamps
    bool debug_regions = false;
    DevArray<unsigned long long> d_stats;   // [kStatSlots][kStWords] sharded counters (zeroed)
    rl::BatchCtl* h_ctl = nullptr;          // pinned copy of the last batch's ctl

    // host-API staging (device copies of caller buffers), all of s_key's size
    DevArray<uint64_t> s_key;
    DevArray<int32_t> s_permits;
    DevArray<int64_t> s_now;
    DevArray<uint16_t> s_lim;
    DevArray<uint8_t> s_op;
    DevArray<uint8_t> s_allowed;
    DevArray<int64_t> s_remaining;
    DevArray<double> s_tokens;
    std::vector<std::pair<void*, size_t>> pinned;   // caller buffers registered by rl_pin_host

    // routing scratch
    DevArray<uint32_t> route_scratch;
    DevArray<uint32_t> route_counts;        // [64]
    DevArray<rl::DirSlot> d_dir;            // hot-key owner directory (empty: hash owners)
    std::vector<rl::DirSlot> h_dir;         // host copy (rl_owner_of_engine)

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
    uint32_t ablate = 0;                    // measurement build: rl_tune("ablate"); else 0
    uint32_t sc_per_cu = 0, un_per_cu = 0;  // rl_tune("*_per_cu"), 0 = default
    uint32_t sc_split = 1;                  // rl_tune("scatter_split"): k_scatter_split
    uint32_t un_split = 2;                  // rl_tune("unpermute_split"): k_unpermute_split
    uint32_t mid_xcd = 0;                   // rl_tune("mid_xcd"): k_unpermute_mid blocks XCD-aware (measured slower)
                                            // 0 off, 1 on, 2 two-pass batches (measured faster there)
    bool force_wide = false;                // rl_tune("wide_records"): 32-B records (any time span)
    bool auto_grow = true;                  // !RL_OPT_FIXED_CAPACITY
    uint32_t inject_fail = 0;               // rl_tune("fail_batches"): tests of callers' error paths
    uint64_t grows = 0;                     // region-count doublings done (rl_batch_stats)
    DevArray<unsigned long long> retry_dbg; // measurement builds (RL_RETRY_COUNT): k_retry_after's counters
    DevArray<int64_t> quota_out;            // [2][n] reset / retry of the host form of rl_quota, on first use
    DevArray<uint8_t> topk;                 // rl_top_keys scratch (topk_scratch_bytes), on first use
    DevArray<unsigned long long> tally;     // [kTallyRows][kTallyWords] the host form of rl_tally_batch, on first use
    DevArray<uint8_t> usage;                // rl_limiter_usage / rl_top_consumers scratch, on first use
    uint32_t usage_passes = 0;              // table passes of the last rl_top_consumers (rl_debug_fetch)
    DevArray<rl::BucketDigest> digest;      // the host form of rl_limiter_digest, largest so far
    DevArray<rl::BucketDigest> digest_fine; // [2^kDigestFineBits] the pass' output when fewer buckets are asked for
    uint32_t digest_per_cu = 0;             // rl_tune("digest_per_cu"), 0 = default
    DevArray<uint8_t> snap;                 // snapshot / ordered-put scratch (snap_scratch_bytes), on first use
    DevArray<uint32_t> put_heads;           // run heads of an ordered put
    DevArray<rl::KeyImage> img_stage;       // images of rl_snapshot_keys / rl_restore_keys / rl_check_images
    DevArray<unsigned long long> check_rep; // [kCrWords] the host forms' report of rl_check_*, on first use
    // string-key staging of rl_hash_keys / rl_execute_batch_keys, on first use
    size_t key_stage_bytes = (size_t)4 << 20;   // rl_tune("key_stage_bytes"): the blob stage's size
    DevArray<uint8_t> ks_blob;              // one chunk of key bytes
    DevArray<uint64_t> ks_off;              // [keys + 1] offsets
    DevArray<uint64_t> ks_hash;             // [keys] rl_hash_keys' hashes
    DevArray<unsigned long long> ks_hdr;    // [2] the chunks' headers (the host checked the offsets)
    bool keys_direct = false;               // rl_tune("keys_direct"): k_hash_keys' direct path only
    // the small-batch path (rl_small.hpp, run_small in rl_engine_batch.cpp), on first use
    uint64_t small_batch = 0;               // rl_tune("small_batch"): batches up to this size ask for it; 0 = off
    uint64_t small_taken = 0, small_declined = 0;   // rl_small_batches
    bool last_small = false;                // the last batch ran on the path: its ctl carries no hot / walk hint
    DevArray<rl::RecC> sm_rec;              // [small_rec_count()] records in region order
    DevArray<uint32_t> sm_res;              // [small_rec_count()] packed results
    DevArray<int64_t> sm_ext;               // [small_rec_count()] escaped remainders
    DevArray<double> sm_tok;                // [small_rec_count()] balances
    DevArray<uint32_t> sm_rstart, sm_rend;  // [n_regions] the touched regions' runs
    DevArray<uint32_t> sm_order;            // [n_regions + 1] the touched list, its length last
    DevArray<rl::BatchCtl> sm_ctl;          // the path's control block
    DevArray<unsigned long long> sm_stats;  // [kStWords] the one workgroup's counters
    uint8_t* sm_block = nullptr;            // page-locked, mapped: the host form's requests and results (small_block)
};

// rl_engine.cpp
int upload_limiters(rl_engine* e);
int grow_once(rl_engine* e, size_t li);
// rl_engine_batch.cpp
int collect_status(rl_engine* e);
int ensure_staging(rl_engine* e, size_t n);
int stage_requests(rl_engine* e, size_t n, const uint64_t* key, const int32_t* permits,
                   const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op_or_skip);
int run_staged_batch(rl_engine* e, size_t n, bool limiter, bool op, uint8_t* allowed,
                     int64_t* remaining, double* tokens_after);
void small_decline_keys(rl_engine* e, size_t n);   // rl_small_batches' `declined`, for rl_execute_batch_keys

#pragma GCC visibility pop
