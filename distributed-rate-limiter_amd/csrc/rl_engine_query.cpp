// rl_engine_query.cpp — the read-only queries of an engine: retry-after, quota, heavy-hitter keys, the
// batch report, the census of a limiter's table, string keys, the table digest and the table check.
#include "rl_engine_impl.hpp"
#include "rl_check.hpp"
#include "rl_keys.hpp"
#include "rl_report.hpp"

using namespace rl;

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
        if (e->retry_dbg.reserve(3) != RL_OK) return RL_E_NOMEM;
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

// ---------------------------------------------------------------- quota queries
// One launch of k_quota, ordered and isolated as run_retry_device's launch is.
static_assert(RL_QUOTA_INVALID == kQuotaInvalid, "quota: invalid marker");
static int run_quota_device(rl_engine* e, size_t n, const uint64_t* key, const int64_t* now_ns,
                            const uint16_t* limiter, const int32_t* permits, const uint8_t* skip,
                            int64_t* remaining, int64_t* reset_ms, int64_t* retry_ms) {
    QuotaArgs qa{};
    qa.key = key; qa.now_ns = now_ns; qa.limiter = limiter; qa.permits = permits; qa.skip = skip;
    qa.remaining = remaining; qa.reset_ms = reset_ms; qa.retry_ms = retry_ms;
    qa.lims = e->d_lims; qa.n = (uint32_t)n; qa.n_lim = (uint32_t)e->lims.size();
    qa.shard_bits = e->shard_bits;
    HIP_OK(launch_quota(qa, e->stream));
    return RL_OK;
}

// permits and retry_ms come together, and skip only with them
static bool quota_args_ok(const uint64_t* key_hash, const int64_t* now_ns, const int32_t* permits,
                          const uint8_t* skip, const int64_t* remaining, const int64_t* reset_ms,
                          const int64_t* retry_ms) {
    if (!key_hash || !now_ns || !remaining || !reset_ms) return false;
    return (permits != nullptr) == (retry_ms != nullptr) && (!skip || permits);
}

extern "C" int rl_quota_device(rl_engine* e, size_t n, const uint64_t* key_hash, const int64_t* now_ns,
                               const uint16_t* limiter, const int32_t* permits, const uint8_t* skip,
                               int64_t* remaining, int64_t* reset_ms, int64_t* retry_ms, void* stream) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (n > e->opts.max_batch) return RL_E_TOO_LARGE;
    if (n == 0) return RL_OK;
    if (!quota_args_ok(key_hash, now_ns, permits, skip, remaining, reset_ms, retry_ms)) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    StreamJoin join(e->stream, (hipStream_t)stream);
    HIP_OK(join.err);
    const int rc = run_quota_device(e, n, key_hash, now_ns, limiter, permits, skip, remaining, reset_ms, retry_ms);
    HIP_OK(join.finish());
    return rc;
}

extern "C" int rl_quota(rl_engine* e, size_t n, const uint64_t* key_hash, const int64_t* now_ns,
                        const uint16_t* limiter, const int32_t* permits, const uint8_t* skip,
                        int64_t* remaining, int64_t* reset_ms, int64_t* retry_ms) {
    if (!e) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (n > e->opts.max_batch) return RL_E_TOO_LARGE;
    if (n == 0) return RL_OK;
    if (!quota_args_ok(key_hash, now_ns, permits, skip, remaining, reset_ms, retry_ms)) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    // the last batch's status first, as rl_retry_after does (it applies a pending table growth)
    const int st = collect_status(e);
    if (st == RL_E_DEVICE) return st;
    int rc = stage_requests(e, n, key_hash, permits, now_ns, limiter, skip);
    if (rc == RL_OK) rc = e->quota_out.reserve(2 * n);               // [reset | retry]
    if (rc != RL_OK) return rc;
    hipStream_t s = e->stream;
    int64_t* const d_reset = e->quota_out;
    int64_t* const d_retry = e->quota_out + n;
    rc = run_quota_device(e, n, e->s_key, e->s_now, limiter ? e->s_lim : nullptr,
                          permits ? e->s_permits : nullptr, skip ? e->s_op : nullptr, e->s_remaining,
                          d_reset, retry_ms ? d_retry : nullptr);
    if (rc != RL_OK) { (void)hipStreamSynchronize(s); return rc; }
    HIP_OK(hipMemcpyAsync(remaining, e->s_remaining, n * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(reset_ms, d_reset, n * 8, hipMemcpyDeviceToHost, s));
    if (retry_ms) HIP_OK(hipMemcpyAsync(retry_ms, d_retry, n * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i)
        if (reset_ms[i] == RL_QUOTA_INVALID) return RL_E_INVALID_REQUEST;
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
    const int rc = e->topk.reserve(topk_scratch_bytes());
    if (rc != RL_OK) return rc;
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

// ---------------------------------------------------------------- batch report
// rl_report.hip (the tally) and the selector passes of rl_topk.hip (top-denied) on the engine
// stream, under the top-keys calls' rules: they read the caller's arrays of a finished batch and
// write the caller's outputs (and their own scratch), nothing else; no collect_status.
static_assert(RL_TALLY_ROWS == kTallyRows && RL_TALLY_UNKNOWN == kTallyUnknown &&
              RL_TALLY_UNKNOWN == RL_MAX_LIMITERS, "tally rows");
static_assert(sizeof(rl_limiter_tally) == kTallyWords * 8 && sizeof(rl_limiter_tally) == 96, "rl_limiter_tally layout");
static_assert(offsetof(rl_limiter_tally, permits_denied) == kTcPermitsDenied * 8 &&
              offsetof(rl_limiter_tally, over_max) == kTcOverMax * 8 &&
              offsetof(rl_limiter_tally, resets) == kTcResets * 8, "rl_limiter_tally field order");
static_assert(RL_REMAINING_UNKNOWN == kReportRemUnknown && RL_REMAINING_ERROR == kReportRemError &&
              RL_OP_ACQUIRE == 0 && RL_OP_PEEK == 1 && RL_OP_RESET == 2, "report constants");
constexpr uint64_t kTallyMaxN = 1ULL << 31;
constexpr size_t kTallyBytes = (size_t)kTallyRows * sizeof(rl_limiter_tally);

static bool tally_args_ok(size_t n, const int32_t* permits, const uint8_t* allowed, const int64_t* remaining,
                          const rl_limiter_tally* out, uint32_t flags) {
    return (n == 0 || (permits && allowed && remaining)) && out && !(flags & ~(uint32_t)RL_TALLY_ACCUMULATE);
}

static int tally_enqueue(rl_engine* e, size_t n, const int32_t* permits, const uint16_t* limiter,
                         const uint8_t* op, const uint8_t* allowed, const int64_t* remaining,
                         unsigned long long* out) {
    TallyArgs a{};
    a.permits = permits; a.limiter = limiter; a.op = op; a.allowed = allowed; a.remaining = remaining;
    a.out = out; a.n = (uint32_t)n; a.n_lim = (uint32_t)e->lims.size();
    HIP_OK(launch_tally(a, e->stream));
    return RL_OK;
}

extern "C" int rl_tally_batch_device(rl_engine* e, size_t n, const int32_t* permits, const uint16_t* limiter,
                                     const uint8_t* op, const uint8_t* allowed, const int64_t* remaining,
                                     rl_limiter_tally* out, uint32_t flags, void* stream) {
    if (!e) return RL_E_INVALID_ARG;
    if (!tally_args_ok(n, permits, allowed, remaining, out, flags) || ((uintptr_t)out & 7u))
        return RL_E_INVALID_ARG;
    if ((uint64_t)n > kTallyMaxN) return RL_E_TOO_LARGE;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    StreamJoin join(e->stream, (hipStream_t)stream);
    HIP_OK(join.err);
    if (!(flags & RL_TALLY_ACCUMULATE)) HIP_OK(hipMemsetAsync(out, 0, kTallyBytes, e->stream));
    const int rc = tally_enqueue(e, n, permits, limiter, op, allowed, remaining, (unsigned long long*)out);
    if (rc != RL_OK) return rc;
    HIP_OK(join.finish());
    return RL_OK;
}

extern "C" int rl_tally_batch(rl_engine* e, size_t n, const int32_t* permits, const uint16_t* limiter,
                              const uint8_t* op, const uint8_t* allowed, const int64_t* remaining,
                              rl_limiter_tally* out, uint32_t flags) {
    if (!e) return RL_E_INVALID_ARG;
    if (!tally_args_ok(n, permits, allowed, remaining, out, flags)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    // pieces of the staging buffers' size, as rl_top_keys; every piece adds to e->tally
    const size_t chunk = std::min<size_t>(std::max<size_t>(n, 1), (size_t)e->opts.max_batch);
    int rc = ensure_staging(e, chunk);
    if (rc == RL_OK) rc = e->tally.reserve((size_t)kTallyRows * kTallyWords);
    if (rc != RL_OK) return rc;
    hipStream_t s = e->stream;
    if (flags & RL_TALLY_ACCUMULATE) HIP_OK(hipMemcpyAsync(e->tally, out, kTallyBytes, hipMemcpyHostToDevice, s));
    else HIP_OK(hipMemsetAsync(e->tally, 0, kTallyBytes, s));
    for (size_t at = 0; at < n; at += chunk) {
        const size_t m = std::min(chunk, n - at);
        HIP_OK(hipMemcpyAsync(e->s_permits, permits + at, m * 4, hipMemcpyHostToDevice, s));
        if (limiter) HIP_OK(hipMemcpyAsync(e->s_lim, limiter + at, m * 2, hipMemcpyHostToDevice, s));
        if (op) HIP_OK(hipMemcpyAsync(e->s_op, op + at, m, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(e->s_allowed, allowed + at, m, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(e->s_remaining, remaining + at, m * 8, hipMemcpyHostToDevice, s));
        rc = tally_enqueue(e, m, e->s_permits, limiter ? e->s_lim.p : nullptr, op ? e->s_op.p : nullptr,
                           e->s_allowed, e->s_remaining, e->tally);
        if (rc != RL_OK) { (void)hipStreamSynchronize(s); return rc; }
    }
    HIP_OK(hipMemcpyAsync(out, e->tally, kTallyBytes, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return RL_OK;
}

// The selector over staged or caller arrays for limiter `sel` (checked by the caller).
static TopkSel topk_sel(const rl_engine* e, const int32_t* permits, const uint16_t* limiter, const uint8_t* op,
                        const uint8_t* allowed, const int64_t* remaining, uint16_t sel) {
    TopkSel s{};
    s.permits = permits; s.limiter = limiter; s.op = op; s.allowed = allowed; s.remaining = remaining;
    s.n_lim = (uint32_t)e->lims.size(); s.sel = sel;
    return s;
}

extern "C" int rl_top_denied_device(rl_engine* e, size_t n, const uint64_t* key_hash, const int32_t* permits,
                                    const uint16_t* limiter, const uint8_t* op, const uint8_t* allowed,
                                    const int64_t* remaining, uint16_t sel_limiter, uint32_t k,
                                    uint64_t min_count, uint64_t* top_key, uint64_t* top_count,
                                    uint64_t* hdr, void* stream) {
    if (!topk_args_ok(e, n, key_hash, k, min_count) || !top_key || !top_count || !hdr ||
        (n && (!permits || !allowed || !remaining)))
        return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (sel_limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    TopkScratch sc;
    int rc = topk_scratch(e, &sc);
    if (rc != RL_OK) return rc;
    const TopkSel sel = topk_sel(e, permits, limiter, op, allowed, remaining, sel_limiter);
    hipStream_t s = e->stream;
    StreamJoin join(s, (hipStream_t)stream);
    HIP_OK(join.err);
    HIP_OK(launch_topk_clear(sc, s));
    HIP_OK(launch_topk_pass_sel(sc, 0, key_hash, sel, (uint32_t)n, min_count, s));
    HIP_OK(launch_topk_pass_sel(sc, 1, key_hash, sel, (uint32_t)n, min_count, s));
    HIP_OK(launch_topk_select(sc, k, min_count, n, top_key, top_count, hdr, s, true));
    HIP_OK(join.finish());
    return RL_OK;
}

extern "C" int rl_top_denied(rl_engine* e, size_t n, const uint64_t* key_hash, const int32_t* permits,
                             const uint16_t* limiter, const uint8_t* op, const uint8_t* allowed,
                             const int64_t* remaining, uint16_t sel_limiter, uint32_t k, uint64_t min_count,
                             uint64_t* top_key, uint64_t* top_count, size_t* n_out, uint64_t* n_heavy,
                             uint64_t* n_denied) {
    if (!topk_args_ok(e, n, key_hash, k, min_count) || !top_key || !top_count || !n_out || !n_heavy ||
        (n && (!permits || !allowed || !remaining)))
        return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (sel_limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    TopkScratch sc;
    int rc = topk_scratch(e, &sc);
    if (rc != RL_OK) return rc;
    const size_t chunk = std::min<size_t>(std::max<size_t>(n, 1), (size_t)e->opts.max_batch);
    rc = ensure_staging(e, chunk);
    if (rc != RL_OK) return rc;
    const TopkSel sel = topk_sel(e, e->s_permits, limiter ? e->s_lim.p : nullptr, op ? e->s_op.p : nullptr,
                                 e->s_allowed, e->s_remaining, sel_limiter);
    hipStream_t s = e->stream;
    HIP_OK(launch_topk_clear(sc, s));
    for (int pass = 0; pass < 2; ++pass)
        for (size_t at = 0; at < n; at += chunk) {
            const size_t m = std::min(chunk, n - at);
            HIP_OK(hipMemcpyAsync(e->s_key, key_hash + at, m * 8, hipMemcpyHostToDevice, s));
            HIP_OK(hipMemcpyAsync(e->s_permits, permits + at, m * 4, hipMemcpyHostToDevice, s));
            if (limiter) HIP_OK(hipMemcpyAsync(e->s_lim, limiter + at, m * 2, hipMemcpyHostToDevice, s));
            if (op) HIP_OK(hipMemcpyAsync(e->s_op, op + at, m, hipMemcpyHostToDevice, s));
            HIP_OK(hipMemcpyAsync(e->s_allowed, allowed + at, m, hipMemcpyHostToDevice, s));
            HIP_OK(hipMemcpyAsync(e->s_remaining, remaining + at, m * 8, hipMemcpyHostToDevice, s));
            HIP_OK(launch_topk_pass_sel(sc, pass, e->s_key, sel, (uint32_t)m, min_count, s));
        }
    HIP_OK(launch_topk_select(sc, k, min_count, n, sc.out_key, sc.out_cnt, sc.out_hdr, s, true));
    uint64_t hdr[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(hdr, sc.out_hdr, sizeof(hdr), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    *n_out = 0;
    *n_heavy = 0;
    if (n_denied) *n_denied = hdr[3];
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
    const int rc = e->usage.reserve(usage_scratch_bytes());
    if (rc != RL_OK) return rc;
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
    if (e->ks_blob.cap != e->key_stage_bytes) e->ks_blob.free();   // (a smaller stage too)
    int rc = e->ks_blob.reserve(e->key_stage_bytes);
    if (rc == RL_OK) rc = e->ks_hdr.reserve(2);
    if (rc == RL_OK) rc = e->ks_off.reserve(keys + 1);
    if (rc == RL_OK) rc = e->ks_hash.reserve(keys);
    return rc;
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
    small_decline_keys(e, n);                          // (the keys are hashed into the staging arrays)
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
        const int rc = e->digest_fine.reserve((size_t)1 << kDigestFineBits);
        if (rc != RL_OK) return rc;
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
    int rc = e->digest.reserve(nb);
    if (rc != RL_OK) return rc;
    rc = digest_enqueue(e, limiter, now_ns, bucket_bits, flags, e->digest);
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

// ---------------------------------------------------------------- table check
// rl_check.hip on the engine stream, under the census' rules (above): behind every batch
// submitted before, the table as installed, no collect_status, nothing written but the report
// (e->check_rep: the host forms' device-side report).
static_assert(RL_CHECK_CLASSES == kCheckClasses && sizeof(rl_check_report) == kCrWords * 8 &&
              sizeof(rl_check_report) == 312, "rl_check_report layout");
static_assert(offsetof(rl_check_report, used_slots) == kCrUsed * 8 &&
              offsetof(rl_check_report, bad_slots) == kCrBad * 8 &&
              offsetof(rl_check_report, violations) == kCrViolations * 8 &&
              offsetof(rl_check_report, first) == kCrFirst * 8, "rl_check_report field order");
static_assert(RL_CHECK_WRONG_REGION == kCkWrongRegion && RL_CHECK_UNREACHABLE == kCkUnreachable &&
              RL_CHECK_DUPLICATE == kCkDuplicate && RL_CHECK_DEAD_MARK == kCkDeadMark &&
              RL_CHECK_SW_START == kCkSwStart && RL_CHECK_SW_COUNT == kCkSwCount &&
              RL_CHECK_SW_OFFSET == kCkSwOffset && RL_CHECK_TB_FLAGS == kCkTbFlags &&
              RL_CHECK_TB_TOKENS == kCkTbTokens && RL_CHECK_IMAGE_LIMITER == kCkImageLimiter &&
              RL_CHECK_IMAGE_RESERVED == kCkImageReserved, "check class ids");
constexpr uint32_t kCheckMinBits = kBinShift, kCheckMaxBits = 24;

// The report set up and the pass over regions [begin, begin + count), clipped to the 2^bits
// regions at `tab`, with limiter li's constants: both on the engine stream.
static int check_enqueue(rl_engine* e, size_t li, const void* tab, const uint64_t* xtab, uint32_t bits,
                         uint64_t begin, uint64_t count, unsigned long long* out) {
    const DevLimiter& L = e->lims[li].dev;
    const uint64_t total = 1ULL << bits;
    CheckArgs a{};
    a.tab = (const Slot*)tab; a.xtab = xtab;
    a.region_begin = begin;
    a.m = begin >= total ? 0 : std::min<uint64_t>(count, total - begin);
    a.region_bits = (int32_t)bits; a.shard_bits = e->shard_bits;
    a.algo = L.algo; a.window_ms = L.window_ms; a.ttl_ms = L.ttl_ms;
    a.out = out;
    HIP_OK(launch_check_init(out, a.m, a.m * kRegionSlots, e->stream));
    HIP_OK(launch_check_regions(a, e->stream));
    return RL_OK;
}

// (e->mu held) limiter li's own table; RL_E_INTERNAL if it is not 2^region_bits regions
static int check_own_enqueue(rl_engine* e, size_t li, uint64_t begin, uint64_t count, unsigned long long* out) {
    const HostLimiter& h = e->lims[li];
    const uint32_t bits = (uint32_t)h.dev.region_bits;
    if (h.table_bytes != ((size_t)kRegionSlots * sizeof(Slot)) << bits) return RL_E_INTERNAL;
    return check_enqueue(e, li, h.table, (const uint64_t*)h.cache_table, bits, begin, count, out);
}

extern "C" int rl_check_limiter_device(rl_engine* e, uint16_t limiter, uint64_t region_begin,
                                       uint64_t region_count, rl_check_report* out_dev, void* stream) {
    if (!e || !out_dev || ((uintptr_t)out_dev & 7u)) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    StreamJoin join(e->stream, (hipStream_t)stream);
    HIP_OK(join.err);
    const int rc = check_own_enqueue(e, limiter, region_begin, region_count, (unsigned long long*)out_dev);
    if (rc != RL_OK) return rc;
    HIP_OK(join.finish());
    return RL_OK;
}

extern "C" int rl_check_limiter(rl_engine* e, uint16_t limiter, uint64_t region_begin,
                                uint64_t region_count, rl_check_report* out) {
    if (!e || !out) return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    int rc = e->check_rep.reserve(kCrWords);
    if (rc != RL_OK) return rc;
    rc = check_own_enqueue(e, limiter, region_begin, region_count, e->check_rep);
    if (rc != RL_OK) return rc;
    rl_check_report r;
    HIP_OK(hipMemcpyAsync(&r, e->check_rep, sizeof(r), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    *out = r;
    return RL_OK;
}

extern "C" int rl_check_table_device(rl_engine* e, uint16_t limiter, const void* slots,
                                     const uint64_t* cache_words, uint32_t region_bits,
                                     rl_check_report* out_dev, void* stream) {
    if (!e || !slots || !out_dev || ((uintptr_t)slots & 15u) || ((uintptr_t)cache_words & 7u) ||
        ((uintptr_t)out_dev & 7u) || region_bits < kCheckMinBits || region_bits > kCheckMaxBits)
        return RL_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mu);
    if (limiter >= e->lims.size()) return RL_E_INVALID_ARG;
    (void)hipSetDevice(e->device);
    StreamJoin join(e->stream, (hipStream_t)stream);
    HIP_OK(join.err);
    const int rc = check_enqueue(e, limiter, slots, cache_words, region_bits, 0, 1ULL << region_bits,
                                 (unsigned long long*)out_dev);
    if (rc != RL_OK) return rc;
    HIP_OK(join.finish());
    return RL_OK;
}

static int check_images_enqueue(rl_engine* e, size_t n, const KeyImage* in, uint64_t index_base,
                                unsigned long long* out) {
    CheckImgArgs a{};
    a.in = in; a.n = n; a.index_base = index_base;
    a.lims = e->d_lims; a.n_lim = (uint32_t)e->lims.size();
    a.out = out;
    HIP_OK(launch_check_images(a, e->stream));
    return RL_OK;
}

extern "C" int rl_check_images_device(rl_engine* e, size_t n, const rl_key_image* in,
                                      rl_check_report* out_dev, void* stream) {
    if (!e || !out_dev || ((uintptr_t)out_dev & 7u) || (n && !in) || ((uintptr_t)in & 15u))
        return RL_E_INVALID_ARG;
    if ((uint64_t)n > kCheckMaxImages) return RL_E_TOO_LARGE;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    StreamJoin join(e->stream, (hipStream_t)stream);
    HIP_OK(join.err);
    HIP_OK(launch_check_init((unsigned long long*)out_dev, 0, n, e->stream));
    const int rc = check_images_enqueue(e, n, (const KeyImage*)in, 0, (unsigned long long*)out_dev);
    if (rc != RL_OK) return rc;
    HIP_OK(join.finish());
    return RL_OK;
}

extern "C" int rl_check_images(rl_engine* e, size_t n, const rl_key_image* in, rl_check_report* out) {
    if (!e || !out || (n && !in)) return RL_E_INVALID_ARG;
    if ((uint64_t)n > kCheckMaxImages) return RL_E_TOO_LARGE;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    // pieces of at most max_batch images through e->img_stage, as rl_restore_keys; every piece
    // adds to the one report
    const size_t piece = std::min<size_t>(n, (size_t)std::max<uint64_t>(e->opts.max_batch, 1));
    int rc = e->check_rep.reserve(kCrWords);
    if (rc == RL_OK) rc = e->img_stage.reserve(piece);
    if (rc != RL_OK) return rc;
    hipStream_t s = e->stream;
    HIP_OK(launch_check_init(e->check_rep, 0, n, s));
    for (size_t at = 0; at < n; at += piece) {
        const size_t m = std::min(piece, n - at);
        HIP_OK(hipMemcpyAsync(e->img_stage, in + at, m * sizeof(KeyImage), hipMemcpyHostToDevice, s));
        rc = check_images_enqueue(e, m, e->img_stage, at, e->check_rep);
        if (rc != RL_OK) { (void)hipStreamSynchronize(s); return rc; }
    }
    rl_check_report r;
    HIP_OK(hipMemcpyAsync(&r, e->check_rep, sizeof(r), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    *out = r;
    return RL_OK;
}
