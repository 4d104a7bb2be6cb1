// In-process transport for router tests: G ranks run as threads of one process on one GPU,
// and all_to_all_v is a rendezvous plus device-to-device copies. Every rank publishes its
// send buffer, waits until all have, pulls its own part out of each peer's buffer, and waits
// again so that no peer reuses a buffer that is still being read.
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/rl_engine.h"

namespace looptest {

class Hub {
  public:
    explicit Hub(int world) : world_(world), slots_(world) {}
    int world() const { return world_; }

    struct Slot {
        const char* send = nullptr;
        const uint64_t* off = nullptr;
        const uint64_t* bytes = nullptr;
    };

    void publish(int rank, const Slot& s) { slots_[rank] = s; }
    const Slot& slot(int rank) const { return slots_[rank]; }

    // all ranks meet here; reusable
    void meet() {
        std::unique_lock<std::mutex> lk(mu_);
        const uint64_t round = round_;
        if (++waiting_ == world_) {
            waiting_ = 0;
            ++round_;
            cv_.notify_all();
        } else {
            cv_.wait(lk, [&] { return round_ != round; });
        }
    }

  private:
    int world_;
    std::vector<Slot> slots_;
    std::mutex mu_;
    std::condition_variable cv_;
    int waiting_ = 0;
    uint64_t round_ = 0;
};

struct Endpoint {
    Hub* hub;
    int rank;
};

inline int all_to_all_v(void* ctx, const void* send, const uint64_t* send_off, const uint64_t* send_bytes,
                        void* recv, const uint64_t* recv_off, const uint64_t* recv_bytes, void* stream) {
    Endpoint* ep = static_cast<Endpoint*>(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    bool ok = hipStreamSynchronize(s) == hipSuccess;             // what I send is complete
    ep->hub->publish(ep->rank, {static_cast<const char*>(send), send_off, send_bytes});
    ep->hub->meet();
    for (int p = 0; p < ep->hub->world(); ++p) {
        const Hub::Slot& from = ep->hub->slot(p);
        const uint64_t nb = recv_bytes[p];
        if (from.bytes[ep->rank] != nb) { ok = false; continue; }   // the two sides disagree
        if (nb == 0) continue;
        ok = hipMemcpyAsync(static_cast<char*>(recv) + recv_off[p], from.send + from.off[ep->rank], nb,
                            hipMemcpyDeviceToDevice, s) == hipSuccess && ok;
    }
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    ep->hub->meet();
    return ok ? 0 : -1;
}

inline rl_transport transport(Endpoint* ep) { return rl_transport{ep, all_to_all_v}; }

}  // namespace looptest
