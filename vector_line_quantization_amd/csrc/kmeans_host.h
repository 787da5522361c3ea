// The sequential host parts of Clustering::train that kmeans_api.hip and pq_train_api.hip share: the reference's generator, the
// head of its permutation and the empty-cluster splits decided from the counts.  Host-only, no device call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace vlq_detail {

// RandomGenerator on Linux (utils.cpp:135-155): random_r over an 8-byte state, the LCG on 31 bits; a seed of 0 becomes 1
struct Lcg {
    uint32_t s;
    explicit Lcg(int64_t seed) : s((uint32_t)seed ? (uint32_t)seed : 1u) {}
    int rand_int() { s = (s * 1103515245u + 12345u) & 0x7fffffffu; return (int)s; }
    float rand_float() { return rand_int() / float(1L << 31); }
};

// the first m entries of rand_perm(perm, n, seed) (utils.cpp:307-317): step i only moves entries at or behind i
inline void rand_perm_head(std::vector<int>& perm, int64_t n, int64_t m, int64_t seed) {
    perm.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) perm[(size_t)i] = (int)i;
    Lcg rng(seed);
    for (int64_t i = 0; i + 1 < n && i < m; i++) std::swap(perm[(size_t)i], perm[(size_t)(i + rng.rand_int() % (int)(n - i))]);
}

// utils.cpp:1415-1447 on the counts: the pairs (ci, cj) in their order, the counts after them
inline int plan_splits(std::vector<int64_t>& count, int64_t n, std::vector<int>& pairs) {
    const size_t k = count.size();
    Lcg rng(1234);
    pairs.clear();
    for (size_t ci = 0; ci < k; ci++) {
        if (count[ci] != 0) continue;
        size_t cj = 0;
        for (;; cj = (cj + 1) % k) {
            const float p = (float)(((double)(size_t)count[cj] - 1.0) / (float)(size_t)(n - (int64_t)k));
            if (rng.rand_float() < p) break;
        }
        pairs.push_back((int)ci);
        pairs.push_back((int)cj);
        count[ci] = count[cj] / 2;
        count[cj] -= count[ci];
    }
    return (int)(pairs.size() / 2);
}

}  // namespace vlq_detail
