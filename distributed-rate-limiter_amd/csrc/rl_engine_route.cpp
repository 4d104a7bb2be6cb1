// rl_engine_route.cpp — what a multi-GPU router asks of its engine: the owner partition, the
// pack / fold / unpack kernels of an exchange, the owner directory, the rl::engine_* accessors
// and the synthetic traces.
#include <cmath>

#include "rl_engine_impl.hpp"

using namespace rl;

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
    if (e->route_scratch.reserve(need) != RL_OK || e->route_counts.reserve(64) != RL_OK) return RL_E_NOMEM;
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
        e->d_dir.free();
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
    if (e->d_dir.reserve(kDirSlots) != RL_OK) return RL_E_NOMEM;
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
    if (e->route_scratch.reserve(need) != RL_OK || e->route_counts.reserve(64) != RL_OK) return RL_E_NOMEM;
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
