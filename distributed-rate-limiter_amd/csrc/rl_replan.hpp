// rl_replan.hpp — the host-only arithmetic of a directory re-plan (rl_router_replan_directory,
// rl_router.cpp): which keys change owner between two directories, and the images a rank copied
// grouped by their new owner. Plain C++ (no HIP), so tests/cpp/test_replan_plan.cpp checks it on
// the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

namespace rl {

struct DirPlan {                          // a directory: key[i] is owned by owner[i]
    std::vector<uint64_t> key;
    std::vector<uint32_t> owner;
};

struct Mover { uint64_t key; uint32_t from, to; };

// The movers of a re-plan from directory D to D': the keys of D ∪ D' whose owner differs (a key
// a directory does not list has its hash owner home(key)), ascending, with both owners. Every
// rank derives the same list from the same D and D'. A key listed twice takes its last entry,
// as rl_set_owner_directory does.
template <class Home>
std::vector<Mover> mover_list(const DirPlan& d_old, const DirPlan& d_new, Home home) {
    std::map<uint64_t, Mover> m;
    auto at = [&](uint64_t key) -> Mover& {
        auto it = m.find(key);
        if (it == m.end()) {
            const uint32_t h = home(key);
            it = m.emplace(key, Mover{key, h, h}).first;
        }
        return it->second;
    };
    for (size_t i = 0; i < d_old.key.size(); ++i) at(d_old.key[i]).from = d_old.owner[i];
    for (size_t i = 0; i < d_new.key.size(); ++i) at(d_new.key[i]).to = d_new.owner[i];
    std::vector<Mover> out;
    for (const auto& kv : m)
        if (kv.second.from != kv.second.to) out.push_back(kv.second);
    return out;
}

// The keys of M that `rank` owns under D (ascending, as M is).
inline std::vector<uint64_t> movers_from(const std::vector<Mover>& M, uint32_t rank) {
    std::vector<uint64_t> out;
    for (const Mover& m : M)
        if (m.from == rank) out.push_back(m.key);
    return out;
}

// Images (anything with a key_hash member) of movers, reordered by new owner with their order
// kept inside each owner; returns the images bound for each of the `world` owners. Every image's
// key must be in M.
template <class Img>
std::vector<uint64_t> group_by_new_owner(std::vector<Img>* imgs, const std::vector<Mover>& M,
                                         uint32_t world) {
    auto to = [&](uint64_t key) {
        auto it = std::lower_bound(M.begin(), M.end(), key,
                                   [](const Mover& m, uint64_t k) { return m.key < k; });
        return it->to;                     // (M is ascending by key and holds the key)
    };
    std::stable_sort(imgs->begin(), imgs->end(),
                     [&](const Img& x, const Img& y) { return to(x.key_hash) < to(y.key_hash); });
    std::vector<uint64_t> count(world, 0);
    for (const Img& im : *imgs) ++count[to(im.key_hash)];
    return count;
}

}  // namespace rl
