// The host arithmetic of rl_router_replan_directory (csrc/rl_replan.hpp) on the CPU: the mover
// list between two directories against a brute-force owner comparison, and the grouping of
// copied images by new owner. No engine, no GPU.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "../../distributed-rate-limiter_amd/csrc/rl_replan.hpp"

using namespace rl;

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::printf("FAILED %s (%s:%d)\n", #x, __FILE__, __LINE__);     \
            return 1;                                                       \
        }                                                                   \
    } while (0)

namespace {
struct Img { uint64_t key_hash; uint32_t limiter; };

uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint64_t rnd() {                                    // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

uint32_t owner_under(const DirPlan& d, uint64_t key, uint32_t world) {
    uint32_t o = (uint32_t)(key % world);           // the test's hash owner
    for (size_t i = 0; i < d.key.size(); ++i)
        if (d.key[i] == key) o = d.owner[i];        // (the last entry wins)
    return o;
}

DirPlan random_dir(size_t n, uint64_t key_space, uint32_t world) {
    DirPlan d;
    std::set<uint64_t> seen;
    while (d.key.size() < n) {
        const uint64_t k = rnd() % key_space;
        if (!seen.insert(k).second) continue;
        d.key.push_back(k);
        d.owner.push_back((uint32_t)(rnd() % world));
    }
    return d;
}
}  // namespace

int main() {
    for (uint32_t world : {1u, 2u, 8u, 64u}) {
        auto home = [&](uint64_t k) { return (uint32_t)(k % world); };
        for (int round = 0; round < 20; ++round) {
            const uint64_t space = round % 2 ? 300 : 1ULL << 40;     // overlapping / disjoint directories
            const DirPlan a = random_dir(round == 0 ? 0 : 1 + rnd() % 200, space, world);
            const DirPlan b = random_dir(round == 1 ? 0 : 1 + rnd() % 200, space, world);
            const std::vector<Mover> M = mover_list(a, b, home);
            // brute force over the union
            std::set<uint64_t> uni(a.key.begin(), a.key.end());
            uni.insert(b.key.begin(), b.key.end());
            size_t want = 0;
            for (uint64_t k : uni) want += owner_under(a, k, world) != owner_under(b, k, world);
            CHECK(M.size() == want);
            for (size_t i = 0; i < M.size(); ++i) {
                CHECK(i == 0 || M[i - 1].key < M[i].key);            // ascending, no duplicates
                CHECK(M[i].from == owner_under(a, M[i].key, world));
                CHECK(M[i].to == owner_under(b, M[i].key, world));
                CHECK(M[i].from != M[i].to && M[i].from < world && M[i].to < world);
            }
            // D -> D moves nothing; D -> {} sends every key that is not at home back
            CHECK(mover_list(a, a, home).empty());
            for (const Mover& m : mover_list(a, DirPlan{}, home)) CHECK(m.to == home(m.key));
            // every rank's share of M, its images grouped by new owner
            size_t shares = 0;
            for (uint32_t rank = 0; rank < world; ++rank) {
                const std::vector<uint64_t> mine = movers_from(M, rank);
                shares += mine.size();
                std::vector<Img> imgs;                                // sorted by (limiter, key) as rl_copy_keys
                for (uint32_t lim = 0; lim < 3; ++lim)
                    for (uint64_t k : mine)
                        if ((k + lim) % 3 != 0) imgs.push_back(Img{k, lim});
                const size_t n_img = imgs.size();
                const std::vector<uint64_t> cnt = group_by_new_owner(&imgs, M, world);
                CHECK(cnt.size() == world && imgs.size() == n_img);
                size_t pos = 0;
                for (uint32_t o = 0; o < world; ++o) {
                    if (o == rank) CHECK(cnt[o] == 0);                // a mover never stays
                    for (uint64_t j = 0; j < cnt[o]; ++j, ++pos) {
                        CHECK(owner_under(b, imgs[pos].key_hash, world) == o);
                        if (j) {                                      // order kept inside an owner
                            const Img &p = imgs[pos - 1], &q = imgs[pos];
                            CHECK(p.limiter < q.limiter || (p.limiter == q.limiter && p.key_hash < q.key_hash));
                        }
                    }
                }
                CHECK(pos == n_img);
            }
            CHECK(shares == M.size());
        }
    }
    std::printf("replan plan: ok\n");
    return 0;
}
