/*
 * rl_engine.h — C-ABI of the MI355X batched rate-limit decision engine.
 *
 * This is the drop-in boundary that replaces the reference's
 * algorithm + storage pair beneath its unchanged Java `RateLimiter` interface:
 *
 *   reference interface                                  replaced by
 *   ---------------------------------------------------  -----------------------------
 *   RateLimiter.tryAcquire(String)                        rl_try_acquire_batch (permits=1)
 *     core/RateLimiter.java:16
 *   RateLimiter.tryAcquire(String,int)                    rl_try_acquire_batch
 *     core/RateLimiter.java:26
 *     algorithms/SlidingWindowRateLimiter.java:85-131
 *     algorithms/TokenBucketRateLimiter.java:105-143 (+ Lua :38-68)
 *   RateLimiter.getAvailablePermits(String)               rl_available
 *     core/RateLimiter.java:35, SlidingWindowRateLimiter.java:133-137,
 *     TokenBucketRateLimiter.java:145-151
 *   RateLimiter.reset(String)                             rl_reset
 *     core/RateLimiter.java:43, SlidingWindowRateLimiter.java:139-153,
 *     TokenBucketRateLimiter.java:153-158
 *   new SlidingWindowRateLimiter(storage, config, reg)    rl_add_limiter(RL_ALGO_SLIDING_WINDOW, ...)
 *     SlidingWindowRateLimiter.java:46-78
 *   new TokenBucketRateLimiter(storage, config, reg)      rl_add_limiter(RL_ALGO_TOKEN_BUCKET, ...)
 *     TokenBucketRateLimiter.java:70-97
 *   RateLimitConfig.validate()                            rl_add_limiter argument checks
 *     core/RateLimitConfig.java:46-56
 *   RedisRateLimitStorage (JedisPool, Redis keyspace)     rl_create / rl_destroy (HBM state table)
 *     storage/RedisRateLimitStorage.java:22-35
 *
 * Everything is plain C: pointers + sizes, no C++ types, no exceptions. Every
 * entry point returns an int status (RL_OK = 0, < 0 on error). The JNI / FFM
 * bindings that a Java maintainer adds on top are shown in INTEGRATION.md.
 *
 * Semantics (bit-exact with the reference):
 *  - key_hash is the 64-bit hash of the String key, rl_key_hash of its UTF-8 bytes
 *    (computed by the caller, or on the device by rl_hash_keys / rl_execute_batch_keys).
 *    State is kept per (limiter id, key_hash).
 *  - now_ns is converted to milliseconds as floorDiv(now_ns, 1e6); the reference
 *    reads System.currentTimeMillis().
 *  - Requests of one batch are applied in array (arrival) order per key.
 *    Sliding-window state requires per-key non-decreasing now_ms (in-order
 *    replay of a wall-clock trace); token-bucket state has no such requirement.
 *  - A denied request never changes state (SlidingWindowRateLimiter.java:104-111,
 *    TokenBucketRateLimiter.java:61-67,110-116).
 */
#ifndef RL_ENGINE_H
#define RL_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RL_ABI_VERSION 3

/* ---- status codes -------------------------------------------------------- */
#define RL_OK                   0
#define RL_E_INVALID_ARG      (-1)  /* bad argument to an entry point; IllegalArgumentException on the Java side */
#define RL_E_INVALID_REQUEST  (-2)  /* >=1 request had permits <= 0 or an unknown limiter id (others were applied) */
#define RL_E_CAPACITY         (-3)  /* a state-table region overflowed; affected requests report RL_REMAINING_ERROR */
#define RL_E_DEVICE           (-4)  /* HIP runtime / device failure; StorageException on the Java side */
#define RL_E_NOMEM            (-5)  /* device or host allocation failed */
#define RL_E_TOO_LARGE        (-6)  /* batch larger than rl_opts.max_batch */
#define RL_E_LIMITERS         (-7)  /* too many limiters / table space exhausted */
#define RL_E_INTERNAL         (-8)  /* a kernel met a state its logic excludes (an engine bug,
                                       not a capacity or input problem): the hot chains' allow
                                       walk found an allow in a chunk it had already decided, or
                                       exceeded its step bound. The batch's results for the keys
                                       involved are suspect; report it as a defect. */

/* ---- algorithms ---------------------------------------------------------- */
#define RL_ALGO_SLIDING_WINDOW 0    /* algorithms/SlidingWindowRateLimiter.java */
#define RL_ALGO_TOKEN_BUCKET   1    /* algorithms/TokenBucketRateLimiter.java   */

/* ---- per-request operation (rl_execute_batch) ----------------------------- */
#define RL_OP_ACQUIRE 0             /* tryAcquire(key, permits)     */
#define RL_OP_PEEK    1             /* getAvailablePermits(key)     */
#define RL_OP_RESET   2             /* reset(key)                   */

/* ---- sentinel values of `remaining` --------------------------------------- */
#define RL_REMAINING_UNKNOWN  (-1)  /* TB permits > maxPermits: "unable to determine" (RateLimiter.java:33) */
#define RL_REMAINING_INVALID  (-2)  /* permits <= 0 or unknown limiter (IllegalArgumentException in Java)   */
#define RL_REMAINING_ERROR    (-3)  /* request not applied: state-table region full (RL_E_CAPACITY)         */

/* ---- limits of this implementation (checked by rl_add_limiter) ------------ */
#define RL_MAX_LIMITERS         255
#define RL_SW_MAX_PERMITS_LIMIT 2147483646LL        /* SW counts kept as u32 */
#define RL_TB_MAX_PERMITS_LIMIT 9007199254740992LL  /* 2^53: Lua numbers are IEEE doubles */
#define RL_MAX_WINDOW_MS        1073741823LL        /* ~12.4 days; bucket offsets kept as i32 */

typedef struct rl_engine rl_engine;

typedef struct rl_opts {
    int32_t  device;            /* HIP device ordinal (-1: current device)                  */
    uint32_t flags;             /* RL_OPT_* bits                                            */
    uint64_t max_batch;         /* largest n accepted by the batch entry points             */
    uint64_t default_capacity;  /* expected live keys per limiter when rl_add_limiter is used */
    uint32_t shard_index;       /* multi-GPU: this engine owns keys with owner(h) == shard   */
    uint32_t shard_count;       /* multi-GPU: number of shards (power of two, 1 = no sharding) */
    int64_t  max_skew_ms;       /* how far a request may lag behind the earliest request of an
                                   EARLIER batch (front-ends with skewed clocks); state is kept
                                   until it is dead that long before a batch's earliest now.
                                   0: batches arrive in global time order */
} rl_opts;

#define RL_OPT_STAGE_TIMING 0x1u  /* record hipEvents around every stage (rl_stage_times) */
/* Pipelined device batches: the partition of a batch (stages 1-3) runs on a second engine
 * stream into one of two scratch sets, so it overlaps the previous batch's decision stage;
 * decisions are still applied in submission order. It applies to rl_execute_batch_device
 * calls with stream == NULL, whose inputs must then be complete when the call is made
 * (results are complete when rl_sync / rl_last_status return). Calls with a stream and the
 * host-buffer calls are ordered as without the option. Scratch memory doubles. */
#define RL_OPT_PIPELINE     0x2u
/* Fixed-size state tables. By default a limiter's table grows on demand, as the Redis
 * keyspace does (RedisRateLimitStorage.java:38-49): when a batch leaves one of its regions
 * more than 62.5 % full (or overflows one: those requests report RL_REMAINING_ERROR and the
 * batch RL_E_CAPACITY), the region count doubles (twice after an overflow) when the batch's
 * status is collected (rl_last_status, the host-buffer calls). */
#define RL_OPT_FIXED_CAPACITY 0x4u

#define RL_LIM_LOCAL_CACHE 0x1u  /* RateLimitConfig.enableLocalCache (RateLimitConfig.java:37-38) */

typedef struct rl_limiter_config {
    int32_t  algo;              /* RL_ALGO_*                                                  */
    uint32_t flags;             /* RL_LIM_* bits                                              */
    int64_t  max_permits;       /* RateLimitConfig.maxPermits (RateLimitConfig.java:19)       */
    int64_t  window_ms;         /* RateLimitConfig.window.toMillis() (RateLimitConfig.java:24) */
    double   refill_per_s;      /* RateLimitConfig.refillRate (RateLimitConfig.java:31); TB only */
    uint64_t capacity;          /* expected live keys (table sizing); 0 = rl_opts.default_capacity */
    int64_t  local_cache_ttl_ms;/* RateLimitConfig.localCacheTtl (RateLimitConfig.java:43-44);
                                   with RL_LIM_LOCAL_CACHE on a sliding window the engine
                                   emulates SlidingWindowRateLimiter's Caffeine cache
                                   (:57-64,93-121,148-150) deterministically in trace time:
                                   expireAfterWrite(ttl) at ms resolution, no size eviction
                                   (exact while <= 10k keys are cached, maximumSize(10000)).
                                   Token buckets have no cache (TokenBucketRateLimiter). */
} rl_limiter_config;

typedef struct rl_batch_stats {
    uint64_t n;                 /* requests in the last batch                                 */
    uint64_t allowed;           /* requests allowed                                           */
    uint64_t distinct_keys;     /* U: distinct (limiter, key) touched (for the roofline)      */
    uint64_t invalid;           /* requests rejected as invalid                               */
    uint64_t capacity_errors;   /* requests not applied because a region was full            */
    uint64_t regions_touched;   /* state-table regions loaded + written back                  */
    uint64_t table_bytes;       /* state-table bytes read + written by the batch (whole 8 KB
                                   region images both ways; sparse regions: the 128-B buckets
                                   faulted in + the 32-B slots written back)                  */
    uint64_t cache_hits;        /* SW local-cache rejections (ratelimiter.cache.hits,
                                   SlidingWindowRateLimiter.java:75-77,96)                  */
    uint64_t table_grows;       /* region-count doublings so far (on-demand table growth)   */
    uint64_t hot_regions;       /* regions decided by the hot-key chains in the last batch   */
    uint64_t routed;            /* requests of the last batch routed straight to their final
                                   partition in pass 0 (the previous batch's hot regions)    */
} rl_batch_stats;

/* Create / destroy an engine on one GPU. Replaces the JedisPool + Redis keyspace
 * (RedisRateLimitStorage.java:22-35). */
int  rl_create(const rl_opts* opts, rl_engine** out);
void rl_destroy(rl_engine* e);

/* Register a limiter; mirrors the constructors SlidingWindowRateLimiter.java:46-78 /
 * TokenBucketRateLimiter.java:70-97 (config.validate() + refillRate > 0 for TB).
 * The id is the `limiter` value used in the batch calls. */
int  rl_add_limiter(rl_engine* e, int algo, int64_t max_permits, int64_t window_ms,
                    double refill_per_s, uint16_t* id);
int  rl_add_limiter_ex(rl_engine* e, const rl_limiter_config* cfg, uint16_t* id);

/* Grow a limiter's state table (doubling its regions, live state kept) until it holds
 * min_keys keys at load <= 0.5; rl_limiter_slots reports its current slot count. */
int  rl_grow_limiter(rl_engine* e, uint16_t limiter, uint64_t min_keys);
int  rl_limiter_slots(rl_engine* e, uint16_t limiter, uint64_t* slots);

/* tryAcquire over a batch of HOST buffers (pageable or pinned).
 *   allowed[i]      1 if request i acquired its permits
 *   remaining[i]    SW: max(0, max - estimate) at now_i after applying request i
 *                   TB: (long) token balance returned by the Lua script, -1 if permits > max
 *   tokens_after[i] TB: the fp64 balance returned by the script (NaN otherwise); may be NULL
 * `limiter` may be NULL (all requests use limiter 0). Returns RL_E_INVALID_REQUEST if
 * any request was invalid (those report RL_REMAINING_INVALID; the rest are applied). */
int  rl_try_acquire_batch(rl_engine* e, size_t n,
                          const uint64_t* key_hash, const int32_t* permits,
                          const int64_t* now_ns, const uint16_t* limiter,
                          uint8_t* allowed, int64_t* remaining, double* tokens_after);

/* Page-lock (hipHostRegister) a caller-owned host buffer that is reused across batches,
 * so the host-buffer entry points above and below DMA it directly instead of staging it
 * through pageable bounce buffers (the JNI side pins its direct ByteBuffers once, see
 * INTEGRATION.md). Already page-locked memory is accepted as is. rl_unpin_host must be
 * called before the buffer is freed; rl_destroy unpins whatever is left. */
int  rl_pin_host(rl_engine* e, void* ptr, size_t bytes);
int  rl_unpin_host(rl_engine* e, void* ptr);

/* Mixed operations (RL_OP_*) over host buffers; `op` may be NULL (all ACQUIRE). */
int  rl_execute_batch(rl_engine* e, size_t n,
                      const uint64_t* key_hash, const int32_t* permits,
                      const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op,
                      uint8_t* allowed, int64_t* remaining, double* tokens_after);

/* Same as rl_execute_batch on DEVICE-resident buffers, enqueued on `stream`
 * (a hipStream_t; NULL = the engine's stream). Asynchronous: results are ready
 * when the stream completes; the status of the batch is then available from
 * rl_last_status(). Used by bench.py and the multi-GPU router (HBM-resident data). */
int  rl_execute_batch_device(rl_engine* e, size_t n,
                             const uint64_t* key_hash, const int32_t* permits,
                             const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op,
                             uint8_t* allowed, int64_t* remaining, double* tokens_after,
                             void* stream);
int  rl_last_status(rl_engine* e);     /* synchronises the engine stream */

/* getAvailablePermits for n keys at now_ns[i] (host buffers). SW: max(0, max - estimate).
 * TB: (long) min(cap, tokens + elapsed*rate) without consuming (the reference's TB
 * getAvailablePermits is broken). */
int  rl_available(rl_engine* e, uint16_t limiter, size_t n, const uint64_t* key_hash,
                  const int64_t* now_ns, int64_t* available);

/* reset(key) for n keys at now_ns[i]: SW deletes the current and previous window
 * buckets; TB deletes the bucket. */
int  rl_reset(rl_engine* e, uint16_t limiter, size_t n, const uint64_t* key_hash,
              const int64_t* now_ns);

/* ---- retry-after for denied acquires ------------------------------------------
 * For query i = (limiter, key_hash, permits, now_ns) with now = floorDiv(now_ns, 1e6) and S the
 * key's state when the call runs (after every batch submitted before it), let P(t) be
 * "tryAcquire(key, permits) at millisecond t is allowed on S" (not applied; with
 * RL_LIM_LOCAL_CACHE the local cache's rejecting entry counts). Then
 *   wait_ms[i] = min{ t >= now : P(t) } - now      (0: allowed right now; an absent or expired
 *                                                   key gives 0 for any permits <= maxPermits)
 *              = RL_RETRY_NEVER    permits > maxPermits (TokenBucketRateLimiter.java:110-116;
 *                                  a sliding window's estimate is never negative)
 *              = RL_RETRY_INVALID  permits <= 0 or unknown limiter (the host-buffer call then
 *                                  returns RL_E_INVALID_REQUEST; the other queries are answered)
 * exactly: the engine's own decision code evaluates P. wait_ms <= 2 * window_ms +
 * local_cache_ttl_ms + 1. skip[i] != 0 gives wait_ms[i] = 0 without a table access, so a
 * batch's own arrays and its `allowed` output can be handed straight back and only the
 * denials cost a lookup. The call changes nothing: no state, no cache entry, no batch
 * statistic, not the status rl_last_status reports. A sliding-window query whose now lies
 * before the key's newest INCR (time regression) is searched from that INCR's time; its wait
 * still counts from now. Multi-GPU: ask the key's owner, as with the batch calls
 * (rl_router_retry_after does that for a whole batch of queries, collectively).
 * `limiter` and `skip` may be NULL (limiter 0, nothing skipped). */
#define RL_RETRY_NEVER   (-1)
#define RL_RETRY_INVALID (-2)
int  rl_retry_after(rl_engine* e, size_t n, const uint64_t* key_hash, const int32_t* permits,
                    const int64_t* now_ns, const uint16_t* limiter, const uint8_t* skip,
                    int64_t* wait_ms);
/* The same on DEVICE buffers, enqueued on `stream` (NULL = the engine's stream) behind every
 * batch submitted before it; returns launch / argument status only. */
int  rl_retry_after_device(rl_engine* e, size_t n, const uint64_t* key_hash,
                           const int32_t* permits, const int64_t* now_ns,
                           const uint16_t* limiter, const uint8_t* skip,
                           int64_t* wait_ms, void* stream);

/* ---- quota: remaining, exact reset and retry-after in one lookup ---------------------
 * The numbers of X-RateLimit-Remaining, X-RateLimit-Reset and Retry-After for a batch of
 * responses, across limiters, from one table lookup per key (X-RateLimit-Limit is the
 * limiter's configured maxPermits). For query i = (limiter, key_hash, now_ns) with
 * now = floorDiv(now_ns, 1e6), S the key's state when the call runs (after every batch
 * submitted before it) and A(t) what RL_OP_PEEK / rl_available reads at millisecond t on S:
 *   remaining[i] = A(now)                                    (bit-equal to rl_available)
 *   reset_ms[i]  = min{ t >= now : A(t) == maxPermits } - now
 *                  the wait until the key's full quota is back; 0 for an absent or expired key.
 *                  It always exists: reset_ms <= 2 * window_ms + 1 for a now not before the
 *                  key's newest write. The local cache does not count, as in
 *                  getAvailablePermits. Exact: the engine's own decision code evaluates A, and
 *                  a returned t is one it confirmed at t and refuted at t - 1.
 *   retry_ms[i]  = what rl_retry_after answers for (limiter, key_hash, permits[i], now_ns[i])
 *                  (the cache counts, RL_RETRY_NEVER for permits > maxPermits); only when
 *                  `permits` and `retry_ms` are both given. skip[i] != 0 gives retry_ms[i] = 0
 *                  without a search; remaining and reset_ms are still answered, and a skipped
 *                  query's permits is not looked at.
 * reset_ms is not retry_ms of permits = maxPermits when the limiter has a local cache: a
 * rejecting cache entry delays an acquire, not the quota. A sliding-window query whose now lies
 * before the key's newest INCR (time regression) with A(now) < maxPermits is searched from that
 * INCR's time, as in rl_retry_after.
 * `permits` without `retry_ms`, `retry_ms` without `permits` and `skip` without `permits` are
 * RL_E_INVALID_ARG. An unknown limiter, or a non-skipped query with permits[i] <= 0, writes
 * RL_QUOTA_INVALID to every output of that query; the host-buffer call then returns
 * RL_E_INVALID_REQUEST with the other queries answered. n and the other arguments are checked
 * as in rl_retry_after. The call changes nothing: no state, no cache entry, no batch statistic,
 * not the status rl_last_status reports. Multi-GPU: ask the key's owner. */
#define RL_QUOTA_INVALID (-2)
int  rl_quota(rl_engine* e, size_t n, const uint64_t* key_hash, const int64_t* now_ns,
              const uint16_t* limiter, const int32_t* permits, const uint8_t* skip,
              int64_t* remaining, int64_t* reset_ms, int64_t* retry_ms);
/* The same on DEVICE buffers, enqueued on `stream` (NULL = the engine's stream) behind every
 * batch submitted before it; returns launch / argument status only. */
int  rl_quota_device(rl_engine* e, size_t n, const uint64_t* key_hash, const int64_t* now_ns,
                     const uint16_t* limiter, const int32_t* permits, const uint8_t* skip,
                     int64_t* remaining, int64_t* reset_ms, int64_t* retry_ms, void* stream);

/* ---- heavy-hitter keys of a key stream ------------------------------------------
 * The candidates rl_router_plan_directory asks for, computed on the device: with
 * c(h) = #{ i < n : key_hash[i] == h } and H = { h : c(h) >= min_count }, ordered by c
 * descending and then key_hash ascending as an unsigned 64-bit value,
 *   n_heavy = |H| (exact, also when it exceeds k),  n_out = min(k, n_heavy),
 *   top_key / top_count [0, n_out) = the first n_out elements of H with their exact counts;
 * entries at and beyond n_out are left untouched. Ties at the cut are broken by that order, so
 * the answer is unique. Every 64-bit value is a legal key, 0 and ~0 included. There is no
 * approximate mode: a result reported without overflow is exact.
 * RL_E_INVALID_ARG, before any device call and with every output untouched: a null engine,
 * n > 0 with a null key_hash, a null output pointer, k == 0, k > RL_TOP_KEYS_MAX,
 * min_count == 0, n > 2^31. n == 0 is valid (n_out = n_heavy = 0).
 * Overflow: a count sketch (2 rows of 2^22 cells) drops the keys that cannot reach min_count,
 * and the others, up to 4 x RL_TOP_KEYS_CANDIDATES of them, are counted exactly. The call
 * reports overflow when n_heavy > RL_TOP_KEYS_CANDIDATES (always) or when more keys than the
 * store holds pass the sketch; never when the sample has at most RL_TOP_KEYS_CANDIDATES
 * distinct keys. The host form then returns RL_E_CAPACITY with *n_out = *n_heavy = 0 (raise
 * min_count or sample less).
 * Both forms only read: no limiter state, batch statistic or rl_last_status changes. Their
 * scratch (38.8 MiB, whatever n is) is allocated by the first call and freed by rl_destroy.
 * One top-keys call (or top-denied call, below: the same scratch) may be in flight per engine.
 * The host form stages key_hash through the engine's staging buffers in chunks of at most
 * rl_opts.max_batch keys (n itself is not bounded by it) and synchronises. */
#define RL_TOP_KEYS_MAX        4096    /* = the owner directory's capacity                */
#define RL_TOP_KEYS_CANDIDATES 65536   /* most keys that may qualify in one call          */
int  rl_top_keys(rl_engine* e, size_t n, const uint64_t* key_hash, uint32_t k, uint64_t min_count,
                 uint64_t* top_key, uint64_t* top_count, size_t* n_out, uint64_t* n_heavy);
/* The same on DEVICE buffers (key_hash [n], top_key / top_count [k], hdr [4]), enqueued on
 * `stream` (NULL = the engine's stream) without a host synchronisation; returns argument /
 * launch status only. hdr = { n_out, n_heavy, overflow, n }; on overflow { 0, 0, 1, n } and
 * top_key / top_count untouched. */
int  rl_top_keys_device(rl_engine* e, size_t n, const uint64_t* key_hash, uint32_t k,
                        uint64_t min_count, uint64_t* top_key, uint64_t* top_count, uint64_t* hdr,
                        void* stream);

/* ---- batch report: per-limiter counts and the keys being throttled ----------------
 * Two read-only analyses of a FINISHED batch's own arrays: what the caller submitted
 * (permits, limiter, op) and what the engine answered (allowed, remaining). `limiter` and `op`
 * may be NULL (limiter 0, RL_OP_ACQUIRE), as in the batch calls. With L the engine's limiter
 * count, request i has
 *   row   = limiter[i] < L ? limiter[i] : RL_TALLY_UNKNOWN   (ids are 0..254, so row 255 is free)
 *   class = the first that matches of
 *     INVALID  limiter[i] >= L, or op[i] > 2, or op[i] == RL_OP_ACQUIRE and permits[i] <= 0
 *              (the engine's own rule, taken from the inputs: a token bucket's remaining can
 *              legitimately read -2 after a time regression)
 *     ERROR    allowed[i] == 0 and remaining[i] == RL_REMAINING_ERROR
 *     PEEK / RESET  by op[i]
 *     ALLOWED  allowed[i] != 0
 *     DENIED   otherwise; those with remaining[i] == RL_REMAINING_UNKNOWN (token bucket,
 *              permits > maxPermits; a rejection in TokenBucketRateLimiter.java:114) are also
 *              counted in over_max.
 * One ambiguity is inherited from the result encoding: a valid, denied token-bucket acquire whose
 * balance reads exactly -3 after a time regression is counted as ERROR.
 * A row's `allowed` / `denied` are the reference's meters ratelimiter.requests.allowed /
 * .rejected (sliding window) and ratelimiter.tokenbucket.allowed / .rejected (token bucket) of
 * that limiter for this batch.
 *
 * rl_tally_batch: out[RL_TALLY_ROWS], one rl_limiter_tally per row; every row satisfies
 * requests == invalid + errors + allowed + denied + peeks + resets. Without RL_TALLY_ACCUMULATE
 * all 256 rows are overwritten (zeros included, reserved = 0); with it the batch's counts are
 * added to what `out` holds (reserved is left alone), so an exporter can keep cumulative
 * counters on the device and read 24 KB per scrape. All sums are modulo 2^64.
 * The device form is enqueued on `stream` (NULL = the engine's stream) behind every batch
 * submitted before it, without a host synchronisation, and returns argument / launch status
 * only; `out` is DEVICE memory, 8-byte aligned. The host form stages the arrays through the
 * engine's staging buffers in pieces of at most rl_opts.max_batch requests (n itself is not
 * bounded by it) and synchronises. Neither form changes limiter state, cache words,
 * rl_batch_stats or the status rl_last_status reports, and neither collects that status.
 * RL_E_INVALID_ARG, before any device call and with `out` untouched: a null engine, n > 0 with
 * a null permits / allowed / remaining, a null out, unknown flag bits, a device `out` that is
 * not 8-byte aligned. n == 0 is valid. RL_E_TOO_LARGE: n > 2^31 in the device form. */
#define RL_TALLY_ROWS       256
#define RL_TALLY_UNKNOWN    255
#define RL_TALLY_ACCUMULATE 0x1u
typedef struct rl_limiter_tally {   /* 96 bytes */
    uint64_t requests, invalid, errors, allowed, denied, over_max, peeks, resets;
    uint64_t permits_allowed;       /* sum of permits over ALLOWED */
    uint64_t permits_denied;        /* sum of permits over DENIED  */
    uint64_t reserved[2];           /* written as 0 */
} rl_limiter_tally;
int  rl_tally_batch(rl_engine* e, size_t n, const int32_t* permits, const uint16_t* limiter,
                    const uint8_t* op, const uint8_t* allowed, const int64_t* remaining,
                    rl_limiter_tally* out, uint32_t flags);
int  rl_tally_batch_device(rl_engine* e, size_t n, const int32_t* permits, const uint16_t* limiter,
                           const uint8_t* op, const uint8_t* allowed, const int64_t* remaining,
                           rl_limiter_tally* out, uint32_t flags, void* stream);
/* rl_top_denied: who is being throttled. With S = { i : row(i) == sel_limiter and class(i) ==
 * DENIED }, the result is exactly what rl_top_keys defines for the subsequence key_hash[S]: the
 * same order (count descending, then key ascending unsigned), n_heavy / n_out, untouched
 * tails, overflow rule and RL_E_CAPACITY behaviour, and the same k / min_count / n argument
 * checks; n > 0 also needs permits, allowed and remaining, and sel_limiter >= L is
 * RL_E_INVALID_ARG. The device form's hdr = { n_out, n_heavy, overflow, |S| }; the host form
 * returns |S| in *n_denied (nullable). Call rules as rl_top_keys(_device). Both forms use the
 * top-keys scratch: one top-keys OR top-denied call may be in flight per engine. */
int  rl_top_denied(rl_engine* e, size_t n, const uint64_t* key_hash, const int32_t* permits,
                   const uint16_t* limiter, const uint8_t* op, const uint8_t* allowed,
                   const int64_t* remaining, uint16_t sel_limiter, uint32_t k, uint64_t min_count,
                   uint64_t* top_key, uint64_t* top_count, size_t* n_out, uint64_t* n_heavy,
                   uint64_t* n_denied);
int  rl_top_denied_device(rl_engine* e, size_t n, const uint64_t* key_hash, const int32_t* permits,
                          const uint16_t* limiter, const uint8_t* op, const uint8_t* allowed,
                          const int64_t* remaining, uint16_t sel_limiter, uint32_t k,
                          uint64_t min_count, uint64_t* top_key, uint64_t* top_count, uint64_t* hdr,
                          void* stream);

/* Observability. */
int  rl_batch_stats_get(rl_engine* e, rl_batch_stats* out);
/* Milliseconds of each pipeline stage of the last batch (needs RL_OPT_STAGE_TIMING);
 * names[i] are static strings. Returns the number of stages written (<= cap). */
int  rl_stage_times(rl_engine* e, const char** names, float* ms, int cap);
int  rl_sync(rl_engine* e);
/* Tuning / measurement knobs (not needed by callers); an unknown key is RL_E_INVALID_ARG.
 * "ablate" is no key of this library: the kernel variants that are wrong by design exist only
 * in the measurement build (-DRL_MEASURE=1, tools/build_variant.sh), where it is their bit set.
 * "hot_threshold" (records per region for the hot-key chains, 0 = off), "route" (two-pass
 * tables: the previous batch's hot regions skip the second partition pass, default 1),
 * "region_order" (largest regions dispatched first, default 1), "walk" (the hot chains' allow
 * walk, default 1), "walk_min" (keys walked: at least this many allows expected per batch,
 * default 4000), "chain_split" (hot chains as two-wave workgroups, default 1), "group_bits"
 * (two-pass batches: bits of the pass-0 digit, default 12; the local grouping resolves the
 * rest), "segments" (two-pass batches: pass-0 output in that many tile segments, default 1),
 * "tile_items" (partition tile = value x 512 requests; 0 = by batch size), "sparse_max",
 * "stage_timing", "debug_regions" and the "*_per_cu" grid sizes; "key_stage_bytes" (the blob
 * stage of rl_hash_keys / rl_execute_batch_keys, default 4 MiB, at least RL_KEY_MAX_BYTES) and
 * "keys_direct" (the key-hash kernel's workgroups all take the direct-read path, default 0).
 * Every setting gives the same decisions. "fail_batches" = k makes the next k batch
 * calls fail with RL_E_DEVICE before enqueuing anything (tests of callers' error paths);
 * "hot_epoch" = v sets the hot marks' epoch counter as is (tests of its wrap-around); the
 * counter restarts at 0 whenever the marks are (re)allocated (the first hot batch, the first
 * one after the region count grew), so set it after a hot batch on the table in question. */
int  rl_tune(rl_engine* e, const char* key, int64_t value);
/* ---- small batches: one launch, one round trip ----
 * rl_tune(e, "small_batch", v), v > 0: a batch of n <= min(v, RL_SMALL_BATCH_MAX) requests given
 * to rl_execute_batch_device (any stream), rl_execute_batch or rl_try_acquire_batch (and so
 * rl_available and rl_reset) is decided by one kernel launch of one workgroup instead of the
 * pipeline's chain of kernels. The host forms pack the requests into a page-locked block of the
 * engine (allocated by the first such call, sized for RL_SMALL_BATCH_MAX), which the kernel
 * reads and writes in place: one launch and one synchronisation, no copy enqueued. v = 0 (the
 * default) turns the path off; v < 0 is RL_E_INVALID_ARG. Measured (DESIGN.md §4 "Small
 * batches"): one request 33 us instead of 305 us per host call, the path ahead up to n = 256 and
 * behind at 1024 with all-distinct keys, so v = 256 is the value to use. Its scratch (39 KiB
 * and 12 bytes per table region) is allocated by the first batch that takes it and freed by
 * rl_destroy.
 *
 * Identical to the pipeline, bit for bit: allowed, remaining, tokens_after, the returned status
 * and rl_last_status, the limiter state left behind (rl_limiter_digest), table growth and
 * RL_E_CAPACITY, the rejection of a batch that spans more than 2^32 ms (the host forms run it
 * again in 32-byte records on the pipeline, as they always did), entries past n untouched, and
 * rl_batch_stats except two fields that describe the pipeline's own work: hot_regions and
 * routed are 0 after a small batch (no hot chains, no routing: a batch this small is far below
 * their thresholds). The per-key order contract holds: requests of one key in array order.
 * The path leaves the pipeline's hot marks, route list and launch hints as they were.
 *
 * Declined: a batch of eligible size (n <= v) that goes to the pipeline all the same, each
 * counted once in `declined`:
 *  - n > RL_SMALL_BATCH_MAX;
 *  - a router's own batches (rl_router_*: their status is folded from the pipeline's control
 *    block on the device);
 *  - rl_execute_batch_keys (the keys are hashed into the pipeline's staging arrays);
 *  - an engine with RL_OPT_STAGE_TIMING or rl_tune "stage_timing" / "debug_regions" on (the
 *    stamps belong to the pipeline's stages);
 *  - an RL_OPT_PIPELINE engine (the batch would have to be ordered behind the partition
 *    stream's batch in flight; it is declined instead, never reordered);
 *  - 32-byte records: a limiter with max_permits above 4194302, rl_tune "wide_records", and
 *    the second run of a host-form batch that spans more than 2^32 ms (that batch counts once
 *    as taken, for the run that rejected it, and once as declined);
 *  - an engine with no limiter (the pipeline's all-invalid fill answers it).
 * A batch of n > v, and every batch while v = 0, is not counted.
 *
 * rl_small_batches: `taken` = batches decided on the path, `declined` as above, both since
 * rl_create; either pointer may be null. */
#define RL_SMALL_BATCH_MAX 1024
int  rl_small_batches(rl_engine* e, uint64_t* taken, uint64_t* declined);
/* Diagnostics (not needed by callers). "region_times": after a batch run with
 * rl_tune("debug_regions", 1), copies per-bin {t_start, t_end, records, rounds, cycle
 * counters} (uint64 x28 per bin; s_memrealtime ticks; rounds bit 63 = a hot region).
 * Returns the number of bins copied (>= 0) or a status < 0. "usage_passes": one uint32, the
 * table passes of the last rl_top_consumers call (digit passes + the compaction); returns 1.
 * "alloc_probe" (tests of rl_debug_alloc_fill): makes a fresh device allocation of `bytes`
 * bytes (at most 1 MiB) the way every buffer of the library is made, copies it out as it was
 * handed over and frees it; returns `bytes`. */
int  rl_debug_fetch(rl_engine* e, const char* what, void* out, size_t bytes);
/* ---- debug (tests only) ----
 * Process-wide: with byte in 0..255 every device allocation the library makes from then on
 * (engines, limiter tables, routers) is filled with that byte before it is used; -1 (the
 * default) turns the fill off. The library's own initialisations come after the fill. Costs
 * nothing per batch either way; a test of "every word is written before it is read". */
int  rl_debug_alloc_fill(int byte);
const char* rl_strerror(int status);
int  rl_abi_version(void);

/* ---- state export / import in the Redis keyspace layout ----
 * The reference keeps all limiter state in Redis; these two calls move the engine's
 * state in and out in that same layout (checkpoint / migration / hybrid deploys).
 * One entry per live Redis key:
 *   RL_STATE_SW_BUCKET  "rl:<key>:<window_start>" counter
 *                       (SlidingWindowRateLimiter.java:185-188; INCR + PEXPIRE w,
 *                        RedisRateLimitStorage.java:38-49)
 *   RL_STATE_TB_BUCKET  "tb:<key>" hash {tokens, last_refill}
 *                       (TokenBucketRateLimiter.java:46-48,63-64; HMSET + PEXPIRE 2w)
 * expire_at_ms is the PEXPIRE deadline: the key is gone once now > expire_at_ms
 * (SW: last INCR + w; TB: last_refill + 2w). */
#define RL_STATE_SW_BUCKET 0
#define RL_STATE_TB_BUCKET 1
typedef struct rl_state_entry {
    uint64_t key_hash;
    uint16_t limiter;
    uint8_t  kind;              /* RL_STATE_*                                          */
    uint8_t  reserved[5];
    int64_t  window_start_ms;   /* SW: bucket start W (a multiple of w); TB: 0         */
    int64_t  count;             /* SW: counter value (>= 1); TB: 0                     */
    double   tokens;            /* TB: balance, the exact fp64 the Lua script stored   */
    int64_t  last_refill_ms;    /* TB: last_refill; SW: 0                              */
    int64_t  expire_at_ms;      /* PEXPIRE deadline                                    */
} rl_state_entry;               /* 56 bytes */

/* Every key live at now_ns (floorDiv to ms, as the batch calls), sorted by
 * (limiter, key_hash, window_start_ms). *n_out = number of live entries; when it
 * exceeds cap nothing is written and RL_E_TOO_LARGE is returned (retry with a larger
 * buffer). `out` is a host buffer. Only this engine's shard is exported. */
int  rl_export_state(rl_engine* e, int64_t now_ns, rl_state_entry* out, size_t cap,
                     size_t* n_out);
/* Load entries (host buffer) into the state table, replacing the state of every key
 * they name. A key's SW buckets are its newest bucket W and, if present, W - w (older
 * ones can never be read again and are dropped). Entries owned by another shard are
 * skipped; *n_imported (nullable) = entries taken. RL_E_INVALID_ARG: unknown limiter,
 * kind not matching the limiter's algorithm, or a deadline the reference could not
 * have set (TB: expire_at != last_refill + 2w; SW: outside [W + w, W + 2w)).
 * RL_E_CAPACITY: a region had no free slot (the other keys are imported). */
int  rl_import_state(rl_engine* e, const rl_state_entry* in, size_t n, size_t* n_imported);

/* ---- key migration: the state of a listed set of keys, bit for bit ------------------
 * rl_export_state / rl_import_state move a whole keyspace in the Redis layout; these three move
 * exactly the listed keys between engines (a hot-key directory that is re-planned on a live
 * router, rl_router_replan_directory). An image is a key's slot as stored plus its local-cache
 * word, so the receiving engine decides every later request of the key exactly as the sending
 * one would have, a sliding-window key blocked by the local cache included. Images are opaque
 * except key_hash / limiter and valid between engines with identical limiter lists. No `now` is
 * involved: state that is dead by TTL travels as it is.
 * All three take HOST buffers, run on the engine's stream behind every batch submitted before
 * them (RL_OPT_PIPELINE included) and synchronise. They work on the table as installed (a growth
 * the last batch asked for but nobody has collected is not applied, as rl_export_state), change
 * no batch statistic, and neither change nor collect the status rl_last_status reports.
 * RL_E_INVALID_ARG, before any device call and with every output untouched: a null engine
 * (checked first), n > RL_MOVE_KEYS_MAX (copy / drop), n > 0 with a null array, a null n_out,
 * cap > 0 with a null out, an image whose limiter the engine does not have (put). n == 0 is
 * valid. */
#define RL_MOVE_KEYS_MAX 8192               /* old + new directory */
typedef struct rl_key_image {               /* 48 bytes */
    uint64_t key_hash;
    uint64_t word[3];                       /* the slot's state words as stored */
    uint64_t cache_word;                    /* local-cache word, 0 without a cache table */
    uint16_t limiter;
    uint16_t reserved[3];
} rl_key_image;
/* Read-only. For every listed key (duplicates count once) and every limiter of the engine, one
 * image if the key's slot holds state or a cache word; keys that were reset or never seen give
 * none. Sorted by (limiter, key_hash as an unsigned value). *n_out = the exact count; when it
 * exceeds cap nothing is written and RL_E_TOO_LARGE is returned. */
int  rl_copy_keys(rl_engine* e, size_t n, const uint64_t* key_hash, rl_key_image* out, size_t cap,
                  size_t* n_out);
/* Removes what rl_copy_keys of the same list returns: each such slot becomes a tombstone (it
 * keeps its place in its probe chain until a sweep or a crowded region load reclaims it).
 * *n_dropped (nullable) = slots rewritten. */
int  rl_drop_keys(rl_engine* e, size_t n, const uint64_t* key_hash, uint64_t* n_dropped);
/* Inserts images, each into the region of its limiter that its key hashes to, replacing any
 * state and cache word the key has there. There is no ownership check: the caller vouches that
 * this engine owns the keys (multi-GPU: by hash or by the directory). RL_E_CAPACITY: a region
 * had no free slot; the other images are put. *n_put (nullable) = images put. */
int  rl_put_keys(rl_engine* e, size_t n, const rl_key_image* in, size_t* n_put);

/* ---- snapshot / restore: a whole table as images ------------------------------------
 * rl_copy_keys needs the keys and takes RL_MOVE_KEYS_MAX of them; rl_export_state loses the
 * local-cache word, costs one atomic per slot and sorts on the host. These four move a whole
 * limiter's table as rl_key_image arrays with no sort anywhere (checkpoint an engine, warm a
 * replica, rebuild an engine after a device reset): an engine restored from a snapshot decides
 * every later request exactly as the snapshotted one would have.
 * A key's region is the region_bits bits of mix64(key_hash) below the shard bits, so for a table
 * with fewer region bits k' <= k, region_k' = region_k >> (k - k'): images in the region order of
 * the source are already grouped by region for any destination with the same shard count and at
 * most as many regions. The snapshot emits that order; the device put relies on it.
 * Common rules, as for the census and migration calls. The host forms (rl_snapshot_keys,
 * rl_restore_keys) run on the engine's stream behind every batch submitted before them
 * (RL_OPT_PIPELINE included) and synchronise; the device forms are enqueued behind those batches
 * and return. All four work on the table as installed: a growth the last batch asked for but
 * nobody has collected is not applied, and a put never grows a table (size a fresh destination
 * first with rl_grow_limiter(limiter, regions_total * 128)). The snapshot calls only read: no
 * state, cache word, batch statistic, and not the status rl_last_status reports. None of the four
 * collects that status. RL_E_INVALID_ARG, before any device call and with every output untouched:
 * a null engine (checked first), an unknown limiter (snapshot), a null output or header pointer,
 * cap > 0 with a null out, n > 0 with a null in, a device image array that is not 16-byte aligned
 * (every element of a hipMalloc'ed rl_key_image array is). One snapshot or put may be in flight
 * per engine. Device memory, allocated by the first call and freed by rl_destroy: 8 B per region
 * of a call + 48 B = 512 KiB (a call handles at most 65536 regions, whatever the table's size);
 * 4 B per image of the largest put so far; the host forms' staged images (min(cap, 256 x the
 * regions of the call), or min(n, rl_opts.max_batch), x 48 B).
 * Consistency: a chunk shows the table as it was when the chunk ran. A point-in-time snapshot
 * needs no batch between its chunks; a caller that sees regions_total change between two chunks
 * (the table grew) starts over. */
#define RL_SNAPSHOT_MIN_CAP 256   /* = slots per region: a cap that always makes progress */

/* Images of every slot of `limiter` that holds state or a cache word (the rule of rl_copy_keys:
 * tombstones and free slots give none; no `now`, dead-by-TTL state travels as it is), for the
 * regions [region_begin, region_begin + region_count) clipped to the table, in
 * (region ascending, slot index ascending) order. Whole regions only:
 *   regions_done  = R, the number of leading regions of the range whose images were all written
 *   n_out         = images written = sum of those R regions' counts (<= cap)
 *   regions_total = the limiter's region count when the call ran (rl_limiter_slots / 256)
 * R is the largest prefix of the range's first 65536 regions that fits cap (cap itself counts up
 * to 2^31). R >= 1 whenever cap >= RL_SNAPSHOT_MIN_CAP and the clipped range is not empty; the
 * next chunk starts at region_begin + R.
 * Entries at and beyond n_out are untouched. If even the first region does not fit (only possible
 * with cap < 256): RL_E_TOO_LARGE, regions_done = 0, *n_out = that region's count, nothing written.
 * region_begin >= regions_total: RL_OK with 0 / 0. `out` is a HOST buffer. */
int  rl_snapshot_keys(rl_engine* e, uint16_t limiter, uint64_t region_begin, uint64_t region_count,
                      rl_key_image* out, size_t cap, size_t* n_out, uint64_t* regions_done,
                      uint64_t* regions_total);
/* DEVICE out[cap] and hdr[4] = { n_out, regions_done, regions_total, 0 }; enqueued on `stream`
 * (NULL = the engine's) with no host synchronisation; returns argument / launch status only.
 * The too-large case reads { 0, 0, regions_total, first region's count }. */
int  rl_snapshot_keys_device(rl_engine* e, uint16_t limiter, uint64_t region_begin,
                             uint64_t region_count, rl_key_image* out, size_t cap, uint64_t* hdr,
                             void* stream);

/* rl_put_keys on DEVICE images with no per-image host work: same effect on the table. Each image
 * replaces the key's state and cache word in the region it hashes to; there is no ownership check.
 * Requires ORDERED FORM: (limiter, destination region) non-decreasing over in[0..n).
 * rl_snapshot_keys output has it for a destination whose limiter has the same shard_bits and at
 * most as many regions (chunks of several limiters: in limiter order). Duplicate keys are applied
 * in array order.
 * hdr[4] = { n_put, n_failed, rejected, n }: n_failed = images that found no free slot
 * (the others are put). rejected bit 0 = not in ordered form, bit 1 = an image names a limiter
 * the engine does not have; if rejected != 0 the table is untouched and n_put = 0.
 * RL_E_TOO_LARGE: n > 2^31. */
int  rl_put_keys_device(rl_engine* e, size_t n, const rl_key_image* in, uint64_t* hdr, void* stream);

/* HOST images of any order and any size. Staged to the device in pieces of at most
 * rl_opts.max_batch images. Each piece goes through rl_put_keys_device. A piece that is not in
 * ordered form takes the path of rl_put_keys. Same result and status as rl_put_keys(n, in). */
int  rl_restore_keys(rl_engine* e, size_t n, const rl_key_image* in, size_t* n_put);

/* Background TTL sweep (Redis active expiry of the PEXPIRE deadlines set at
 * RedisRateLimitStorage.java:41-44 and Lua :64): frees every slot none of whose buckets is live at
 * now_ns, so used slots track live keys even for regions no batch touches. (Batches already
 * drop dead slots of the regions they load.) The sweep frees slots, not memory: the allocation
 * keeps its size; rl_shrink_limiter below gives table memory back. now_ns must not exceed the
 * now of any later request, as with Redis's own clock. *reclaimed (nullable) = slots freed. */
int  rl_sweep_expired(rl_engine* e, int64_t now_ns, uint64_t* reclaimed);

/* ---- table shrink: give table memory back after a key flood --------------------------
 * rl_grow_limiter and the automatic growth only ever double a limiter's region count; after a
 * flood of one-off keys has expired, the table (32 B per slot, + 8 B with a local cache) and every
 * slot-proportional pass (sweep, census, export, snapshot) would keep paying for the peak. The
 * reference's Redis returns memory as keys expire; these two calls do it in place, with no second
 * engine and no change to the limiter list.
 * Regions 2r and 2r+1 of a table with k region bits are region r with k-1 bits (the split of
 * rl_grow_limiter, read backwards), so a table halved i times has region r' = the regions
 * r' << i ... (r' << i) + 2^i - 1 merged. With kept(r) = the slots of region r live at now =
 * floorDiv(now_ns, 1e6) (the rule of rl_sweep_expired), fullest[i] is the largest sum of kept
 * over one region of the table halved i times. halvings = j = the largest i < levels with
 *   fullest[i] <= RL_SHRINK_FILL_MAX  and
 *   slots_before >> i >= max(2 * ceil(min_keys / shard_count), 8 * 256)
 * (the load <= 0.5 rule of rl_grow_limiter and the minimum of 8 regions); i = 0, no change, is
 * always allowed. RL_SHRINK_FILL_MAX is half the fill at which a batch flags a limiter for growth
 * (208 of 256 slots): the fullest region of a shrunk table must double its keys before the table
 * grows again.
 * rl_shrink_plan only reads: no state, cache word, batch statistic, and not the status
 * rl_last_status reports (the standing of rl_limiter_usage). rl_shrink_limiter runs the same plan
 * and, if j > 0, installs a table of 2^(k-j) regions holding exactly the kept slots, slot words
 * and local-cache word bit for bit; slots dead at now and tombstones are not carried (a shrink
 * includes that limiter's sweep, and now_ns has the restriction stated there). With j == 0 the
 * table is not touched at all, not even swept, and the call returns RL_OK. *out (nullable for
 * rl_shrink_limiter) receives the plan the call acted on. It works with RL_OPT_FIXED_CAPACITY
 * too: it is an explicit call. Nothing shrinks on its own.
 * Common rules, as for the census and snapshot calls: both run behind every batch submitted before
 * them (RL_OPT_PIPELINE included) and synchronise; they work on the table as installed and neither
 * change nor collect the batch status. A growth flag of an earlier batch that nobody has collected
 * yet may grow the shrunk table once at the next collection: harmless, the table then has twice
 * the room it needs. RL_E_INVALID_ARG, before any device call and with outputs untouched: a null
 * engine (checked first), an unknown limiter, a null out in rl_shrink_plan.
 * All or nothing: the new table is built in fresh allocations (j halvings in ceil(j / 3) passes
 * through intermediate tables, each at most 1/8 of the one before; peak extra device memory =
 * the new table, 1/2^j of the old one, for j <= 3, and less than 1/7 of the old one with the
 * intermediates for j > 3, + 12 B per region of plan scratch);
 * the old table is freed and the limiter record updated only after the last pass has succeeded.
 * On RL_E_NOMEM, RL_E_DEVICE or RL_E_INTERNAL the old table is still installed and intact.
 * Region ids of this and the later limiters change with a shrink as with a growth. */
#define RL_SHRINK_FILL_MAX 104   /* = 208 / 2 */
#define RL_SHRINK_LEVELS   24
typedef struct rl_shrink_report {
    uint64_t slots_before;   /* == rl_limiter_slots when the call ran                         */
    uint64_t slots_after;    /* slots_before >> halvings                                      */
    uint64_t used_before;    /* slots that were not free (live + dead + tombstones)           */
    uint64_t kept;           /* slots live at now (the rule of rl_sweep_expired): carried over */
    uint32_t halvings;       /* j: the region count is / would be divided by 2^j; 0 = no change */
    uint32_t levels;         /* valid entries of fullest = region_bits - 3 + 1                 */
    uint32_t fullest[RL_SHRINK_LEVELS]; /* fullest[i] = most kept slots in one region if the
                                           region count were halved i times (non-decreasing)   */
} rl_shrink_report;
int  rl_shrink_plan(rl_engine* e, uint16_t limiter, int64_t now_ns, uint64_t min_keys,
                    rl_shrink_report* out);
int  rl_shrink_limiter(rl_engine* e, uint16_t limiter, int64_t now_ns, uint64_t min_keys,
                       rl_shrink_report* out);

/* ---- census of a limiter's table --------------------------------------------------
 * What DBSIZE / INFO keyspace / SCAN answer for the reference's Redis, computed on the device in
 * table passes that return a few hundred bytes (rl_export_state moves 56 B per Redis key and
 * sorts on the host). For limiter L and now = floorDiv(now_ns, 1e6):
 *   live key        a key with at least one Redis key live at now, the rule rl_export_state
 *                   applies (SW: a bucket with !(now > last INCR + w); TB: !(now > last_refill + 2w))
 *   available(key)  what RL_OP_PEEK returns for the key at now (SW: max(0, max - estimate); TB:
 *                   the (long) of the refilled balance, negative after time regression), from
 *                   the engine's own decision code, so exact
 *   used(key)       max_permits - clamp(available, 0, max_permits), in [0, max_permits]
 * Both calls only read: no limiter state, cache word, batch statistic, and not the status
 * rl_last_status reports, which they do not collect either. They read the table as installed: a
 * growth the last batch asked for but nobody has collected is not applied (as rl_export_state).
 * They run on the engine's stream behind every batch submitted before them (RL_OPT_PIPELINE
 * included) and synchronise. RL_E_INVALID_ARG, before any device call and with every output
 * untouched: a null engine (checked first), an unknown limiter, a null output pointer, k == 0,
 * k > RL_TOP_KEYS_MAX, min_used < 0. Their scratch (1,147,136 B = 1.09 MiB, whatever the
 * table's size: 32 counters, a 4096-bin digit histogram, RL_USAGE_CANDIDATES + RL_TOP_KEYS_MAX
 * 16-B candidates) is allocated by the first call and freed by rl_destroy. Multi-GPU: an engine
 * reports its own shard; a key has one owner, so the ranks' rl_usage fields add up. */
#define RL_USAGE_BINS 16
typedef struct rl_usage {
    uint64_t slots;          /* == rl_limiter_slots                                      */
    uint64_t used_slots;     /* slots that are not free (live keys + tombstones)          */
    uint64_t live_keys;
    uint64_t redis_keys;     /* entries rl_export_state(now_ns) emits for this limiter   */
    uint64_t exhausted_keys; /* live keys with used == max_permits (tryAcquire(key,1) denied
                                on the Redis state)                                       */
    uint64_t cache_blocked;  /* SW + RL_LIM_LOCAL_CACHE: keys whose cache entry rejects at now
                                (cache word x != 0 && now < x); 0 otherwise              */
    uint64_t used_permits;   /* sum of used(key) over live keys (modulo 2^64)             */
    uint64_t hist[RL_USAGE_BINS]; /* live keys by bin = used == max ? 15 : used * 16 / max
                                     (integer division); sums to live_keys                */
} rl_usage;
/* One pass over the limiter's slots (32 B each, + 8 B with a cache table). */
int  rl_limiter_usage(rl_engine* e, uint16_t limiter, int64_t now_ns, rl_usage* out);
/* The heaviest consumers: M = { live keys with used >= min_used }, ordered by used descending
 * and then key_hash ascending as an unsigned 64-bit value;
 *   n_match = |M| (exact),  n_out = min(k, n_match),
 *   key_hash / used [0, n_out) = the first n_out elements of M;
 * entries at and beyond n_out are left untouched. The answer is unique and always exact: there
 * is no overflow or approximate mode, however many keys tie (every throttled key has used ==
 * max_permits). Method: a most-significant-digit radix select over the composite (used in
 * bit_length(max_permits) bits, then ~key_hash) in 12-bit digits, one table pass per digit,
 * until the bin that holds the k-th key has at most RL_USAGE_CANDIDATES keys; one more pass then
 * fetches that bin and the fewer than k keys above it, and the host orders them. With hashed
 * keys that is 2 or 3 digit passes + 1 (each pass divides a tie by 4096); the worst case, for
 * max_permits = 2^53 and adversarial key hashes, is ceil((54 + 64) / 12) + 1 = 11 passes. The
 * host reads a 32-KB histogram between passes, hence no stream / device-buffer form. */
#define RL_USAGE_CANDIDATES 65536
int  rl_top_consumers(rl_engine* e, uint16_t limiter, int64_t now_ns, uint32_t k, int64_t min_used,
                      uint64_t* key_hash, int64_t* used, size_t* n_out, uint64_t* n_match);

/* ---- table digest: per-bucket fingerprints of a limiter's live state ---------------
 * What DEBUG DIGEST answers for the reference's Redis, per range of the table: is this limiter's
 * state the same as that one's (a replica, a restore, the table after a re-plan or a shrink), and
 * if not, in which buckets do they differ. One read-only pass over the limiter's slots (32 B each,
 * + 8 B of cache word with RL_DIGEST_CACHE), no sort, no per-slot atomic, a few KB back
 * (rl_export_state moves 56 B per Redis key and sorts on the host).
 *
 * The digest is taken over the LOGICAL state at now = floorDiv(now_ns, 1e6), not over the stored
 * bits, as a multiset of entries:
 *   - every entry rl_export_state(now_ns) would emit for this limiter:
 *       sliding window  one per live bucket "rl:<key>:<W>":  kind SW, fields
 *                       (f1, f2, f3) = (window_start_ms, count, expire_at_ms)
 *       token bucket    one per live hash "tb:<key>":        kind TB, fields
 *                       (f1, f2, f3) = (the 64 bits of `tokens` as stored, last_refill_ms,
 *                       expire_at_ms)   (so +0.0 and -0.0 balances differ)
 *   - with RL_DIGEST_CACHE, and only if the limiter has a local cache: one entry of kind CACHE,
 *     fields (x, 0, 0), for every key whose cache word x rejects at now (x != 0 && now < x, the
 *     cache_blocked rule of rl_usage; x is the millisecond at which the entry stops rejecting =
 *     write time + localCacheTtl, kept only for a cached value >= maxPermits).
 * Tombstones, free slots and state dead at now contribute nothing, so the digest does not change
 * under rl_grow_limiter, rl_sweep_expired, rl_shrink_limiter, snapshot / restore, migration or
 * slot placement, and a caller can recompute it from rl_export_state output or from the
 * reference's keyspace.
 *
 * Entry hash. All arithmetic is uint64 and wrapping; signed fields are taken as their two's
 * complement bits; rotl is a 64-bit left rotation; mix64 is the engine's key mixer, the
 * splitmix64 finaliser
 *     mix64(x):  x ^= x >> 30;  x *= 0xbf58476d1ce4e5b9;  x ^= x >> 27;  x *= 0x94d049bb133111eb;
 *                x ^= x >> 31
 * and tag = mix64(key_hash):
 *     u = tag + K[kind];  u = (u ^ f1) * C1;  u = (u ^ rotl(f2, 23)) * C2;  u ^= rotl(f3, 47);
 *     H = mix64(u)
 *   K[SW] = RL_DIGEST_K_SW, K[TB] = RL_DIGEST_K_TB, K[CACHE] = RL_DIGEST_K_CACHE,
 *   C1 = RL_DIGEST_C1, C2 = RL_DIGEST_C2 (all odd, below; fixed: part of the ABI).
 * The limiter id is not hashed: two engines' limiters compare whatever their ids are.
 *
 * Bucket of an entry: bucket = the top bucket_bits bits of tag below the shard bits
 * (bucket_bits == 0: one bucket). A region is the top region_bits of those same bits, so bucket
 * b is the regions [b << (k - g), (b + 1) << (k - g)) of a table with k region bits, for every
 * table with k >= g = bucket_bits: tables of different sizes that hold the same keys give the
 * same digests, and a bucket is a region range rl_snapshot_keys takes. Every table has at least
 * 8 regions (k >= 3). out[b] = { entries digested, sum of H mod 2^64, xor of H } over bucket b's
 * entries; `total` (nullable) = the same over all buckets.
 *
 * What equality means:
 *   - Equal digests at one now mean, up to a 2^-64-class collision, that the two limiters hold
 *     the same Redis keyspace at now (and the same rejecting cache entries with RL_DIGEST_CACHE).
 *   - A digest taken at now_1 that equals one taken earlier at now_0 <= now_1 means the bucket's
 *     live entries are the same set: every key the table has dropped since was dead at now_1. So
 *     a checkpoint chunk of that bucket taken at now_0 still restores to state that decides
 *     identically from now_1 on.
 *   - Expiry alone can make digests differ; the cost is only a chunk snapshotted again.
 *
 * Both calls only read: no limiter state, cache word, batch statistic, and not the status
 * rl_last_status reports, which they do not collect either. They read the table as installed (a
 * growth nobody has collected is not applied) on the engine's stream behind every batch submitted
 * before them (RL_OPT_PIPELINE included). The host form synchronises; the device form is enqueued
 * (joined with `stream` as the other *_device calls) and returns argument or launch status only;
 * all 2^bucket_bits entries of `out` are written on the stream. RL_E_INVALID_ARG, before any device call and with the
 * outputs untouched: a null engine (checked first), an unknown limiter, a null out, flag bits
 * other than RL_DIGEST_CACHE, bucket_bits greater than the limiter's current region bits
 * (log2(rl_limiter_slots / 256)), a device out that is not 8-byte aligned. Multi-GPU: an engine
 * digests its own shard; buckets lie below the shard bits, so shard s of one deployment compares
 * with shard s of another, and the shards' `entries` add up to the unsharded table's. */
#define RL_DIGEST_CACHE 0x1u        /* also digest the local-cache entries that reject at now */
#define RL_DIGEST_K_SW    0x9e3779b97f4a7c15ULL
#define RL_DIGEST_K_TB    0xc2b2ae3d27d4eb4fULL
#define RL_DIGEST_K_CACHE 0x165667b19e3779f9ULL
#define RL_DIGEST_C1      0xff51afd7ed558ccdULL
#define RL_DIGEST_C2      0xc4ceb9fe1a85ec53ULL
typedef struct rl_bucket_digest {   /* 24 bytes */
    uint64_t entries;               /* entries digested in this bucket */
    uint64_t sum;                   /* sum of H(entry) mod 2^64 */
    uint64_t xr;                    /* xor of H(entry) */
} rl_bucket_digest;
int  rl_limiter_digest(rl_engine* e, uint16_t limiter, int64_t now_ns, uint32_t bucket_bits,
                       uint32_t flags, rl_bucket_digest* out /* HOST [2^bucket_bits] */,
                       rl_bucket_digest* total /* nullable: all buckets combined */);
int  rl_limiter_digest_device(rl_engine* e, uint16_t limiter, int64_t now_ns, uint32_t bucket_bits,
                              uint32_t flags, rl_bucket_digest* out /* DEVICE */, void* stream);

/* ---- table check: is this table sound? ---------------------------------------------
 * What redis-check-rdb answers for the reference's Redis: a read-only device pass over a
 * limiter's table (or over a list of images) that counts the slots breaking the rules every
 * kernel relies on, per rule, and reports where the first such slot is. Use it after a restore
 * from a file, a migration or an RL_E_INTERNAL; it repairs nothing.
 * The rules, for region r of a table with k region bits and 256 slots per region; a slot is USED
 * iff its four words and its local-cache word are not all zero:
 *   structural (whatever wrote the table)
 *   RL_CHECK_WRONG_REGION  a used slot whose tag = mix64(key_hash) does not hash to region r
 *                          (shard ownership is not checked: the owner directory moves keys)
 *   RL_CHECK_UNREACHABLE   a used slot s with a free slot in the cyclic range [home(tag), s),
 *                          home = tag & 252: a lookup stops at that free slot, reports the key
 *                          absent, and the key restarts with a full quota
 *   RL_CHECK_DUPLICATE     a used slot whose tag also sits in a used slot of the region with a
 *                          lower index, both holding bucket state, neither of which had expired
 *                          (last write + ttl, ttl = window_ms / 2 x window_ms for a token bucket)
 *                          before the other was last written; n such copies count n - 1. (A key
 *                          that returns after its TTL may leave its expired slot behind the slot
 *                          it claimed: two slots, ordered in time, and no violation.)
 *   RL_CHECK_DEAD_MARK     token bucket: word[2] == 2 (the mark that keeps the dead slot of
 *                          key_hash 0 from reading as free) on any other slot
 *   values (state no entry point produces from inputs it accepts)
 *   RL_CHECK_SW_START      sliding window, state present: newest bucket start % window_ms != 0
 *   RL_CHECK_SW_OFFSET     sliding window: a bucket with a non-zero count whose last-INCR offset
 *                          is outside (-window_ms, window_ms) (negative only for now < 0)
 *   RL_CHECK_TB_FLAGS      token bucket: word[2] has bits other than bit 0 and is not the mark
 *   RL_CHECK_SW_COUNT and RL_CHECK_TB_TOKENS are reserved ids and never reported:
 *   rl_import_state admits any bucket count in [1, 2^32) and any double as a balance, so a count
 *   above max_permits or a balance outside [0, capacity] is not proof of corruption.
 *   image lists only
 *   RL_CHECK_IMAGE_LIMITER   the engine has no limiter with the image's id (its values are not
 *                            checked)
 *   RL_CHECK_IMAGE_RESERVED  a non-zero reserved field
 * A slot may count in several classes; ids without a rule read 0 / ~0.
 *
 * Common rules, as for the census: every call only reads (no limiter state, cache word, batch
 * statistic, and not the status rl_last_status reports, which it does not collect either), works
 * on the table as installed, and runs on the engine's stream behind every batch submitted before
 * it (RL_OPT_PIPELINE included). The host forms synchronise; the device forms are enqueued
 * (joined with `stream` as the other *_device calls, NULL = the engine's) and return argument or
 * launch status only, the whole report being written on the stream. RL_E_INVALID_ARG, before any
 * device call and with the outputs untouched: a null engine (checked first), an unknown limiter,
 * a null report, a device report that is not 8-byte aligned, a device table or image array that
 * is not 16-byte aligned, cache words that are not 8-byte aligned, region_bits outside [3, 24],
 * n > 0 with a null `in`. RL_E_TOO_LARGE: n > 2^31. Device memory: one 312-byte report (and the
 * host form's staged images, min(n, rl_opts.max_batch) x 48 B), allocated by the first call and
 * freed by rl_destroy. Multi-GPU: an engine checks its own shard. */
#define RL_CHECK_CLASSES 16
#define RL_CHECK_WRONG_REGION    0
#define RL_CHECK_UNREACHABLE     1
#define RL_CHECK_DUPLICATE       2
#define RL_CHECK_DEAD_MARK       3
#define RL_CHECK_SW_START        4
#define RL_CHECK_SW_COUNT        5   /* reserved: not checked */
#define RL_CHECK_SW_OFFSET       6
#define RL_CHECK_TB_FLAGS        7
#define RL_CHECK_TB_TOKENS       8   /* reserved: not checked */
#define RL_CHECK_IMAGE_LIMITER   9
#define RL_CHECK_IMAGE_RESERVED 10
typedef struct rl_check_report {            /* 312 bytes */
    uint64_t regions, slots;                /* checked (an image list: 0, n)                      */
    uint64_t used_slots;                    /* == rl_usage.used_slots over the same range          */
    uint64_t state_slots;                   /* slots that hold state or a cache word: the images
                                               rl_snapshot_keys emits for the range                */
    uint64_t tombstones;                    /* used_slots - state_slots                            */
    uint64_t cache_words;                   /* non-zero cache words                                */
    uint64_t bad_slots;                     /* slots with >= 1 violation                           */
    uint64_t violations[RL_CHECK_CLASSES];  /* slots per class                                     */
    uint64_t first[RL_CHECK_CLASSES];       /* lowest region << 8 | slot per class (an image list:
                                               lowest index), ~0: none; region = index in the table */
} rl_check_report;
/* The regions [region_begin, region_begin + region_count) of `limiter`, clipped to the table.
 * region_begin at or beyond the table: RL_OK, a zeroed report with first[] = ~0. One pass over
 * the range's slots (32 B each, + 8 B with a cache table). */
int  rl_check_limiter(rl_engine* e, uint16_t limiter, uint64_t region_begin, uint64_t region_count,
                      rl_check_report* out /* HOST */);
int  rl_check_limiter_device(rl_engine* e, uint16_t limiter, uint64_t region_begin,
                             uint64_t region_count, rl_check_report* out_dev, void* stream);
/* The same pass over a caller-held DEVICE array laid out as a table, 2^region_bits regions of 256
 * slots of 32 bytes {tag, word[3]}, with limiter `limiter`'s constants and the engine's shard
 * bits: a copy of a table someone holds, or a synthetic one. cache_words (nullable): one uint64
 * per slot. Exactly those bytes are read and nothing else; nothing read from them is used as an
 * address, so any contents are safe to check. */
int  rl_check_table_device(rl_engine* e, uint16_t limiter, const void* slots,
                           const uint64_t* cache_words, uint32_t region_bits,
                           rl_check_report* out_dev, void* stream);
/* The value classes over n images, each with its limiter's constants, and the two image classes;
 * first[] holds image indices, regions = 0, slots = n, used_slots = images that are not all zero
 * (tag included), state_slots = those of a known limiter that hold state or a cache word. The
 * structural classes need a table and do not apply. The host form stages pieces of at most
 * rl_opts.max_batch images. */
int  rl_check_images(rl_engine* e, size_t n, const rl_key_image* in /* HOST */, rl_check_report* out);
int  rl_check_images_device(rl_engine* e, size_t n, const rl_key_image* in /* DEVICE */,
                            rl_check_report* out_dev, void* stream);

/* ---- string keys: one definition of the key hash, computed on the host or the device ------
 * key_hash everywhere in this header is rl_key_hash of the String key's UTF-8 bytes: FNV-1a 64
 * followed by mix64, the splitmix64 finaliser (above). All arithmetic is uint64 and wrapping;
 * every byte c is taken as UNSIGNED (0..255):
 *     h = 0xcbf29ce484222325;  for each byte c:  h = (h ^ c) * 0x100000001b3;
 *     rl_key_hash = mix64(h)
 * (0x100000001b3 = 2^40 + 0x1b3). rl_key_hash is pure host code: no GPU and no engine is
 * needed. len == 0 is valid (`bytes` may then be NULL) and there is no length limit. This is
 * the single definition: the C++ mirror's keyHash calls it, and a front-end either calls it
 * too or hands its key bytes to the batch calls below, which compute the same value on the
 * device. Fixed: part of the ABI.
 *
 * A key batch is key_bytes[key_bytes_len] (uint8_t, any alignment) plus key_off[n + 1]
 * (uint64_t, 8-byte aligned): key i is the bytes [key_off[i], key_off[i + 1]), so keys are
 * contiguous and in request order; key_off[0] need not be 0. Key i is WELL-FORMED when
 *     key_off[i] <= key_off[i + 1],  key_off[i + 1] <= key_bytes_len  and
 *     key_off[i + 1] - key_off[i] <= RL_KEY_MAX_BYTES;
 * zero-length keys are legal.
 *
 * rl_hash_keys_device (DEVICE buffers): key_hash[i] = rl_key_hash(key i) for a well-formed
 * key; a malformed key gets key_hash[i] = 0, none of its bytes is read, and it is counted:
 * hdr = { malformed keys, n }, written on the stream by the call itself. Entries at and beyond
 * n are untouched; n == 0 is valid (hdr = {0, 0}); n > 2^31 returns RL_E_TOO_LARGE. Whatever
 * the offsets hold, the kernel reads only 16-byte-aligned granules of key_bytes that contain a
 * byte of a well-formed key. Enqueued on `stream` (NULL = the engine's stream, joined as the
 * other *_device calls) without a host synchronisation; returns argument or launch status
 * only. RL_E_INVALID_ARG, before any device call and with the outputs untouched: a null engine
 * (checked first), n > 0 with a null key_off or key_hash, a null hdr, key_bytes_len > 0 with a
 * null key_bytes, a key_off, key_hash or hdr that is not 8-byte aligned. The call needs no
 * engine scratch, so any number of calls may be in flight. A device-side string batch is this
 * call followed by rl_execute_batch_device, or rl_router_step, on the same stream with
 * key_hash as the key array: there is no fused device form and no router form.
 *
 * rl_hash_keys (HOST buffers): every offset is checked on the host first; any malformed key
 * returns RL_E_INVALID_ARG with nothing written and no device call. The batch is then staged
 * in chunks cut at key boundaries, of at most rl_opts.max_batch keys and at most the blob
 * stage's size in bytes (default 4 MiB; rl_tune("key_stage_bytes", v), v >= RL_KEY_MAX_BYTES so
 * that a chunk always makes progress), the device form runs per chunk, the hashes are copied
 * back and the call synchronises. n is not bounded by max_batch. The stage memory is allocated
 * by the first call and freed by rl_destroy. Buffers registered with rl_pin_host are DMAed
 * directly, as by the other host-buffer calls.
 *
 * Both hash calls only read: no limiter state, cache word, batch statistic, and not the status
 * rl_last_status reports, which they do not collect either.
 *
 * rl_execute_batch_keys (HOST buffers; the call a JNI layer uses for tryAcquire(String, int)
 * batches): the same offset check as rl_hash_keys; n > rl_opts.max_batch returns
 * RL_E_TOO_LARGE. The blob is staged in byte chunks and hashed on the device straight into the
 * engine's staged key array, then exactly the batch rl_execute_batch would run is run: the
 * outputs, the returned status (RL_E_INVALID_REQUEST and RL_E_CAPACITY included),
 * rl_batch_stats, on-demand growth and what rl_last_status reports are those of
 * rl_execute_batch(e, n, H, ...) with H[i] = rl_key_hash(key i). key_hash_out (nullable)
 * receives H: the hash -> client id mapping a front-end keeps for rl_top_consumers. */
#define RL_KEY_MAX_BYTES 4096
uint64_t rl_key_hash(const void* bytes, size_t len);
int  rl_hash_keys_device(rl_engine* e, size_t n, const uint8_t* key_bytes, size_t key_bytes_len,
                         const uint64_t* key_off, uint64_t* key_hash, uint64_t* hdr /* [2] */,
                         void* stream);
int  rl_hash_keys(rl_engine* e, size_t n, const uint8_t* key_bytes, size_t key_bytes_len,
                  const uint64_t* key_off, uint64_t* key_hash);
int  rl_execute_batch_keys(rl_engine* e, size_t n, const uint8_t* key_bytes, size_t key_bytes_len,
                           const uint64_t* key_off, const int32_t* permits, const int64_t* now_ns,
                           const uint16_t* limiter, const uint8_t* op,
                           uint8_t* allowed, int64_t* remaining, double* tokens_after,
                           uint64_t* key_hash_out /* nullable */);

/* ---- multi-GPU routing helpers (device buffers, engine stream) ------------
 * owner(key_hash) is the shard that holds the key's state. rl_route_partition
 * stably partitions a batch by owner: perm[j] = source index of the j-th request
 * in owner order, counts[s] = requests for shard s (host array of shard_count). */
uint32_t rl_owner_of(uint64_t key_hash, uint16_t limiter, uint32_t shard_count);
int  rl_route_partition(rl_engine* e, size_t n, const uint64_t* key_hash,
                        const uint16_t* limiter, uint32_t shard_count,
                        uint32_t* perm, uint64_t* counts_host, void* stream);
/* out[j] = in[perm[j]] for the four request arrays (limiter / limiter_out nullable). */
int  rl_route_pack(rl_engine* e, size_t n, const uint32_t* perm, const uint64_t* key_hash,
                   const int32_t* permits, const int64_t* now_ns, const uint16_t* limiter,
                   uint64_t* key_out, int32_t* permits_out, int64_t* now_out,
                   uint16_t* limiter_out, void* stream);
/* packed[j] = remaining[j] * 2 + allowed[j] (one int64 per decision for the return trip). */
int  rl_route_fold(rl_engine* e, size_t n, const uint8_t* allowed, const int64_t* remaining,
                   int64_t* packed, void* stream);
/* allowed[perm[j]], remaining[perm[j]] = unfold(packed[j]). */
int  rl_route_unpack(rl_engine* e, size_t n, const uint32_t* perm, const int64_t* packed,
                     uint8_t* allowed, int64_t* remaining, void* stream);

/* Compact wire (16 B per request, the default router layout): out in owner order,
 * wire_out[2j] = key_hash, wire_out[2j+1] = (uint32)permits << 32 | (now_ms - base_ms),
 * limiter_out[j] (nullable) = limiter id. hdr (device int64[2]) receives base_ms =
 * floorDiv(now_ns[0], 1e6) - 2^31 and an overflow flag (1: some now_ms outside
 * [base_ms, base_ms + 2^32); the router then sends that step in the wide layout). */
int  rl_route_pack_wire(rl_engine* e, size_t n, const uint32_t* perm, const uint64_t* key_hash,
                        const int32_t* permits, const int64_t* now_ns, const uint16_t* limiter,
                        uint64_t* wire_out, uint16_t* limiter_out, int64_t* hdr, void* stream);
/* Receiver side: m wire records from n_src sources (host arrays: each source's base_ms
 * and request count, in source order, summing to m) -> request SoA for the engine
 * (now_out = now_ms * 1e6; the engine reads now at ms resolution). */
int  rl_route_unwire(rl_engine* e, size_t m, const uint64_t* wire, uint32_t n_src,
                     const int64_t* src_base, const uint64_t* src_count, uint64_t* key_out,
                     int32_t* permits_out, int64_t* now_out, void* stream);
/* Width in bytes (1, 2, 4 or 8) of the engine's packed decision ((remaining + 3) << 1 |
 * allowed) for its current limiter set: 1 B for every maxPermits <= 124. */
int  rl_result_width(rl_engine* e);
/* packed[j] = (remaining[j] + 3) << 1 | (allowed[j] & 1) in `width` bytes (return trip), and
 * its inverse scattered through perm: allowed[perm[j]], remaining[perm[j]].
 * These two calls have no escape mechanism: the pair is exact for remaining in
 * [-3, ((2^(8 width) - 1) >> 1) - 3] (124 at width 1, 32764 at 2, 2^31 - 4 at 4, 2^63 - 4 at
 * 8), which holds every reply of an engine whose rl_result_width is `width` except a
 * token-bucket balance below -3 after time regression. A remaining outside that range is
 * truncated to `width` bytes and comes back as another value, with no error; a caller that may
 * see such values uses rl_route_fold_return / rl_route_unpack_return below. */
int  rl_route_fold_packed(rl_engine* e, size_t n, const uint8_t* allowed, const int64_t* remaining,
                          void* packed, int width, void* stream);
int  rl_route_unpack_packed(rl_engine* e, size_t n, const uint32_t* perm, const void* packed,
                            int width, uint8_t* allowed, int64_t* remaining, void* stream);

/* Segmented return trip (the router's default): the decisions for peer s travel as
 *   [ packed results, seg_counts[s] x width bytes, padded to 8 B ][ exception block ]
 * with exception block = { u64 count, exc_cap x (i64 position, i64 remaining) } listing the
 * results whose remaining does not fit the width (token-bucket balances below -3 after
 * time regression, Lua :56-58). Segment s covers requests [sum(seg_counts[<s]), +seg_counts[s]).
 * The block's count is the segment's true number of such results, also past exc_cap; only the
 * first exc_cap to arrive are listed, in no particular order.
 * rl_route_return_bytes = total bytes of that layout (0 on bad arguments: n_seg 0 or > 64, a
 * width other than 1, 2, 4, 8). A layout of n_seg segments is n_seg one-segment layouts in a
 * row, so the total is also the sum of the one-segment totals.
 * rl_route_unpack_return scatters through perm like rl_route_unpack_packed and adds to
 * *lost (device u32) the escaped results whose block overflowed (they read allowed 0,
 * remaining RL_REMAINING_ERROR). An escaped result that its block lists comes back with its
 * exact remaining and allowed = 0, whatever allowed was folded: that is right for everything an
 * engine emits, since rl_result_width covers max_permits and so only a negative balance, which
 * is never allowed, escapes. Both calls return RL_E_INVALID_ARG, before any device call, for a
 * width other than 1, 2, 4, 8, n_seg 0 or > 64, or seg_counts that do not sum to m / n. */
uint64_t rl_route_return_bytes(uint32_t n_seg, const uint64_t* seg_counts, int width,
                               uint32_t exc_cap);
int  rl_route_fold_return(rl_engine* e, size_t m, const uint8_t* allowed, const int64_t* remaining,
                          void* out, int width, uint32_t n_seg, const uint64_t* seg_counts,
                          uint32_t exc_cap, void* stream);
int  rl_route_unpack_return(rl_engine* e, size_t n, const uint32_t* perm, const void* in, int width,
                            uint32_t n_seg, const uint64_t* seg_counts, uint32_t exc_cap,
                            uint8_t* allowed, int64_t* remaining, uint32_t* lost, void* stream);
/* Hot-key owner directory (at most 4096 keys): key_hash[i] is owned by shard owner[i]
 * instead of its hash owner, in rl_route_partition(_device) and rl_owner_of_engine. With
 * Zipf traffic the hash owner of the top keys carries a multiple of the mean load (the top
 * key alone draws ~11% of all requests at s = 1.1); listing the hottest keys with owners
 * chosen to even the loads out removes that imbalance. Every rank must
 * install the same directory before any state exists for the listed keys. n = 0 clears.
 * That restriction holds for rl_set_owner_directory / rl_router_plan_directory(_sampled) only:
 * rl_router_replan_directory(_sampled) moves the keys' state and is legal on a live router. */
int  rl_set_owner_directory(rl_engine* e, size_t n, const uint64_t* key_hash,
                            const uint32_t* owner);
uint32_t rl_owner_of_engine(rl_engine* e, uint64_t key_hash);
/* rl_route_partition without a host round-trip: counts[s] (int64) land in DEVICE memory at
 * counts_dev[s * counts_stride] (the router's header column), on `stream`. */
int  rl_route_partition_device(rl_engine* e, size_t n, const uint64_t* key_hash,
                               uint32_t shard_count, uint32_t* perm, int64_t* counts_dev,
                               size_t counts_stride, void* stream);
/* rl_route_partition_device restricted to the requests with skip[i] == 0 (skip NULL: none is
 * skipped, the call is rl_route_partition_device): perm[0 .. n_live) is the stable owner order
 * of the live requests, counts_dev[s * counts_stride] the live count for shard s, n_live the sum
 * of the counts; perm[n_live .. n) is not written. The directory is honoured. A caller hands a
 * step's own key array and its `allowed` output as skip, and only the denials are placed. */
int  rl_route_partition_skip_device(rl_engine* e, size_t n, const uint64_t* key_hash,
                                    const uint8_t* skip, uint32_t shard_count, uint32_t* perm,
                                    int64_t* counts_dev, size_t counts_stride, void* stream);
/* Mixed operations on the wire: op rides in the u16 limiter column,
 *   col[j] = min(limiter[perm[j]], 0x3FFF) | min(op[perm[j]], 3) << 14   (limiter / op nullable: 0)
 * RL_MAX_LIMITERS is 255, so an id clamped to 0x3FFF stays unknown and an op clamped to 3 stays
 * invalid: 0x4001 comes out as an unknown limiter, never as limiter 1 with RL_OP_PEEK. */
int  rl_route_fold_ops(rl_engine* e, size_t n, const uint32_t* perm, const uint16_t* limiter,
                       const uint8_t* op, uint16_t* col, void* stream);
/* limiter_out[j] = col[j] & 0x3FFF, op_out[j] = col[j] >> 14; limiter_out may alias col */
int  rl_route_unfold_ops(rl_engine* e, size_t m, const uint16_t* col, uint16_t* limiter_out,
                         uint8_t* op_out, void* stream);
/* The answers of a query exchange back in the caller's order, one launch: wait_ms[i] = 0 where
 * skip[i] != 0 (skip nullable), wait_ms[perm[j]] = back[j] for j < n_live (perm from
 * rl_route_partition_skip_device with the same skip; n_live <= n). */
int  rl_route_unpack_wait(rl_engine* e, size_t n, size_t n_live, const uint32_t* perm,
                          const int64_t* back, const uint8_t* skip, int64_t* wait_ms, void* stream);
/* The four calls above take device buffers, run on `stream` (NULL: the engine's) and return
 * argument or launch status. */

/* ---- multi-GPU router ----------------------------------------
 * The reference's "distribution" is many app instances sharing one Redis
 * (README.md:266-269); here each GPU owns a hash shard of the keyspace and one router per
 * GPU moves every request to its owner and the decision back. A router wraps an engine
 * created with rl_opts.shard_index = rank, shard_count = world (power of two <= 64).
 *
 * Transport: how a router reaches its peers; all buffers are device pointers and every
 * call is enqueued on `stream` (collective: every rank makes the same calls in the same
 * order). all_to_all_v sends send[send_off[p] .. +send_bytes[p]) to peer p and receives
 * peer p's bytes at recv + recv_off[p]; byte counts are host arrays of `world` entries.
 * The RCCL transport (librl_rccl.so, rl_transport_rccl_create) is the product one; tests
 * supply an in-process loopback. Return 0 on success. */
typedef struct rl_transport {
    void* ctx;
    int (*all_to_all_v)(void* ctx, const void* send, const uint64_t* send_off,
                        const uint64_t* send_bytes, void* recv, const uint64_t* recv_off,
                        const uint64_t* recv_bytes, void* stream);
} rl_transport;

typedef struct rl_router rl_router;
typedef struct rl_router_opts {
    size_t max_batch;           /* the largest per-rank n of rl_router_step                    */
    size_t recv_cap;            /* requests an owner decides per exchange round; 0 = min(world,
                                   2) x max_batch; clamped to the engine's rl_opts.max_batch. A
                                   step in which some owner receives more runs in several
                                   rounds (every rank derives the same plan from the header)   */
} rl_router_opts;
/* Every device buffer a step, an execute or a query uses is reserved here (send side ~50 B x
 * max_batch, receive side ~57 B x recv_cap, the return trip, the directory exchange), so none
 * of them allocates between two collectives. rl_router_create = _ex with recv_cap 0. */
int  rl_router_create_ex(rl_engine* e, uint32_t world, uint32_t rank, const rl_transport* t,
                         const rl_router_opts* opts, rl_router** out);
int  rl_router_create(rl_engine* e, uint32_t world, uint32_t rank, const rl_transport* t,
                      size_t max_batch, rl_router** out);
typedef struct rl_router_stats {
    uint64_t steps;             /* rl_router_step calls that reached the header exchange       */
    uint64_t rounds;            /* exchange rounds (== steps unless a step was split)          */
    uint64_t split_steps;       /* steps in which some owner received more than recv_cap       */
    uint64_t max_recv;          /* most requests this rank's engine received in one step       */
    uint64_t header_sync_ns;    /* host time blocked on the per-step header read, summed (it
                                   also waits for this rank's previous step to drain)          */
    uint64_t recv_cap;
    uint64_t reserved_bytes;    /* device bytes reserved by rl_router_create_ex                */
} rl_router_stats;
int  rl_router_stats_get(rl_router* r, rl_router_stats* out);
/* tryAcquire over this rank's slice of the global arrival stream (device buffers; the
 * ranks' slices are ordered by rank). Same results as one engine on the concatenated
 * stream. One host synchronisation per step (the header exchange: RCCL takes its
 * per-peer counts on the host). Errors are collective: a fatal engine error on any rank is
 * returned, once, by EVERY rank's step — the NEXT step for a failure known when the engine
 * call returns (a launch error, an allocation failure), TWO steps later for a batch's
 * data-dependent status (collected at the next step's header exchange, published in the
 * header after it) — or by rl_router_finish. The failed batch's requests read
 * RL_REMAINING_ERROR. The step that returns a fatal error does not process its own batch:
 * all n of its outputs read allowed = 0, remaining = RL_REMAINING_ERROR, so a caller that
 * goes on never mistakes stale decisions for this batch's. The router then goes on.
 * Non-fatal statuses (RL_E_INVALID_REQUEST) are not returned by a step: rl_router_finish
 * reports the worst of them since the previous finish. */
int  rl_router_step(rl_router* r, size_t n, const uint64_t* key_hash, const int32_t* permits,
                    const int64_t* now_ns, const uint16_t* limiter, uint8_t* allowed,
                    int64_t* remaining, void* stream);
/* A step with operations (RL_OP_*; device buffers): allowed[i] / remaining[i] are what
 * rl_execute_batch gives for request i on one unsharded engine fed the ranks' slices
 * concatenated in rank order, step after step; peeks and resets are applied in array order with
 * the acquires of the same key. op > 2 and unknown limiter ids are invalid exactly as on a
 * single engine (RL_REMAINING_INVALID; rl_router_finish reports RL_E_INVALID_REQUEST).
 * rl_router_step(...) is rl_router_execute(..., op = NULL, ...): the same collectives with the
 * same byte counts, error model, statistics and results.
 * `op` is NULL on every rank or on none, and so is `limiter` (a rank with n = 0 passes any
 * non-NULL pointer): both decide which collectives a step makes.
 * op travels in the u16 limiter column (rl_route_fold_ops; the owner decodes it in place with
 * rl_route_unfold_ops), so with op != NULL the column travels even when limiter == NULL
 * (limiter 0), and an execute with op makes exactly as many all_to_all_v calls as a step with
 * limiter, in the compact, wide and split-round modes alike. */
int  rl_router_execute(rl_router* r, size_t n, const uint64_t* key_hash, const int32_t* permits,
                       const int64_t* now_ns, const uint16_t* limiter, const uint8_t* op,
                       uint8_t* allowed, int64_t* remaining, void* stream);
/* Retry-after for this rank's queries (device buffers), collectively: every rank calls it,
 * between steps. wait_ms[i] is what rl_retry_after on one unsharded engine holding all keys'
 * state would answer for query i (RL_RETRY_NEVER and RL_RETRY_INVALID included; 0 for
 * skip[i] != 0); the key's owner answers, directory owners included, with
 * rl_retry_after_device. `limiter` is NULL on every rank or on none; `skip` is local and may be
 * NULL. n <= max_batch, else RL_E_TOO_LARGE before any collective; null arguments as for the
 * step; n = 0 is valid and still takes part in the collectives.
 * Only the queries with skip == 0 travel: 16 B forward in the compact wire (+ 2 B with
 * `limiter`) and 8 B back, so a caller hands a step's arrays and its `allowed` output straight
 * back and the exchange carries the denials only. The wide layout (a source whose travelling
 * queries span more than 2^31 ms either side of now_ns[0], which is the base whether query 0 is
 * skipped or not) and several rounds (an owner receives more than recv_cap queries) as the step.
 * It uses the buffers rl_router_create_ex reserved and allocates nothing.
 * Ordering: behind this rank's previous step, and on each owner behind every batch its engine
 * was given before (rl_retry_after_device's rule, RL_OPT_PIPELINE included).
 * It changes nothing: no limiter state, cache word or batch statistic, not the engine status,
 * not the statuses the router holds for its next header, not rl_router_stats' steps / rounds /
 * split_steps / max_recv; the header row it exchanges carries status 0.
 * Synchronous end: after the return trip the ranks exchange one status row, the call
 * synchronises the stream and returns the worst status of all ranks, the same on every rank:
 * RL_OK or a fatal one. After the header exchange every rank goes through every collective of
 * the call whatever fails locally; an owner whose rl_retry_after_device fails answers
 * RL_RETRY_ERROR for the queries it received. A capacity mismatch between ranks (max_batch /
 * recv_cap) is detected from the header as in the step: every rank returns RL_E_INVALID_ARG
 * and its wait_ms[0..n) all read RL_RETRY_ERROR. Invalid queries do not make the call fail.
 * A query's now may lie before requests the owner has decided since (a rank asks about its own
 * slice after the whole step; the rounds of a split step are separate engine batches): state is
 * kept for such timestamps for rl_opts.max_skew_ms, as for lagging requests, so the answers for
 * a step's own timestamps are those of one unsharded engine when max_skew_ms covers the
 * step's time span. */
#define RL_RETRY_ERROR (-3)   /* query not answered: its owner's call failed (router form only) */
int  rl_router_retry_after(rl_router* r, size_t n, const uint64_t* key_hash, const int32_t* permits,
                           const int64_t* now_ns, const uint16_t* limiter, const uint8_t* skip,
                           int64_t* wait_ms, void* stream);
/* Collective: the worst status of every rank's last batches (all ranks get the same). */
int  rl_router_finish(rl_router* r);
/* Hot-key directory for the whole router (collective, before any state exists for the
 * chosen keys): each rank passes its n candidates (HOST arrays) with their request counts (e.g. the top
 * keys of a sample of its traffic) and the total it sampled; the router merges them, keeps
 * the k hottest and places them on owners by longest-processing-time-first over the
 * owners' expected loads (rl_set_owner_directory on every rank). *placed = keys listed. */
int  rl_router_plan_directory(rl_router* r, size_t n, const uint64_t* key_hash,
                              const uint64_t* count, uint64_t sampled, uint32_t k,
                              uint32_t* placed, void* stream);
/* The same with the candidates taken from a DEVICE sample of this rank's traffic (collective):
 * rl_top_keys_device(n, key_hash, k, min_count) on the rank's engine, its at most
 * RL_TOP_KEYS_MAX results copied to the host, then rl_router_plan_directory with them and
 * sampled = n. A rank whose sample overflowed (RL_TOP_KEYS_CANDIDATES) contributes no
 * candidates, completes the collective and then returns RL_E_CAPACITY; every rank still
 * installs the same directory. */
int  rl_router_plan_directory_sampled(rl_router* r, size_t n, const uint64_t* key_hash,
                                      uint32_t k, uint64_t min_count, uint32_t* placed,
                                      void* stream);
/* The same two calls on a LIVE router (collective, legal at any point between steps): the new
 * directory D' is planned as above and the state of every key whose owner differs between the
 * installed directory D and D' (a key listed in neither has its hash owner) moves to its new
 * owner with rl_copy_keys / rl_put_keys / rl_drop_keys, so the steps after it decide exactly as
 * one engine on the concatenated stream would. n = 0 on every rank clears the directory and
 * sends every listed key home. *placed = keys listed in D'; *moved = images that changed engine,
 * summed over the ranks (the same on every rank); both nullable.
 * The call first waits for this rank's previous step and settles its engine status as the next
 * step would have (it is still returned by the same later step, or by rl_router_finish). Then
 * every rank copies the movers it owns, the ranks exchange a status row (any failure: every
 * rank returns it, nothing has changed), exchange the images, the new owners put them and the
 * ranks exchange a second status row. All OK: the old owners drop their movers and every rank
 * installs D'. Otherwise the new owners drop what they put, D stays installed and every rank
 * returns the worst status (RL_E_CAPACITY: a receiving region of a fixed-capacity table was
 * full). No path leaves a key's state on two engines or on none. Argument errors
 * (RL_E_INVALID_ARG) are returned before any collective, as with the two calls above. */
int  rl_router_replan_directory(rl_router* r, size_t n, const uint64_t* key_hash,
                                const uint64_t* count, uint64_t sampled, uint32_t k,
                                uint32_t* placed, uint64_t* moved, void* stream);
int  rl_router_replan_directory_sampled(rl_router* r, size_t n, const uint64_t* key_hash,
                                        uint32_t k, uint64_t min_count, uint32_t* placed,
                                        uint64_t* moved, void* stream);
void rl_router_destroy(rl_router* r);

/* ---- synthetic traces (bench / tests; deterministic in (seed, index)) ------ */
#define RL_DIST_UNIFORM 0
#define RL_DIST_ZIPF    1
typedef struct rl_trace_spec {
    uint64_t seed;
    uint64_t n_keys;            /* key population                                */
    int32_t  dist;              /* RL_DIST_*                                      */
    int32_t  permits_max;       /* permits uniform in [1, permits_max]            */
    double   zipf_s;            /* Zipf exponent (dist = RL_DIST_ZIPF)            */
    int64_t  t0_ns;             /* first arrival                                  */
    int64_t  span_ns;           /* arrivals evenly spaced over [t0, t0 + span)    */
    uint64_t index_base;        /* global index of element 0 (sharded traces)     */
    uint64_t n_total;           /* total length of the global trace (time axis)  */
    uint16_t n_limiters;        /* limiter ids assigned round-robin by key rank   */
    uint16_t reserved[3];
} rl_trace_spec;
int  rl_synth_trace_device(rl_engine* e, const rl_trace_spec* spec, size_t n,
                           uint64_t* key_hash, int32_t* permits, int64_t* now_ns,
                           uint16_t* limiter, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RL_ENGINE_H */
