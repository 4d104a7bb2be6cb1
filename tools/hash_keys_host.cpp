// Host side of tools/hash_keys_probe.py: rl_key_hash over a whole key batch on `threads` host
// threads (contiguous key ranges), the work a front-end does when it hashes on the CPU. Built by
// the probe into a shared library next to librl_engine.so and called through ctypes.
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

#include "../include/rl_engine.h"

extern "C" void hash_keys_host(const uint8_t* key_bytes, const uint64_t* key_off, size_t n, int threads,
                               uint64_t* key_hash) {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([=] {
            const size_t lo = n * (size_t)t / (size_t)threads, hi = n * (size_t)(t + 1) / (size_t)threads;
            for (size_t i = lo; i < hi; ++i)
                key_hash[i] = rl_key_hash(key_bytes + key_off[i], (size_t)(key_off[i + 1] - key_off[i]));
        });
    for (auto& th : pool) th.join();
}
