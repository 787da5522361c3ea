// Host test of placement_rank / placement_bin (csrc/placement_key.h): the key that sorts queries onto the XCDs.
// Stand-alone: built with -fsanitize=address,undefined by placement_key.mk; the key arrays are heap blocks of exactly
// nprobe / nlist elements, so a read past either end is reported.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "placement_key.h"

static int failures = 0;
#define CHECK_EQ(a, b)                                                                                          \
    do {                                                                                                        \
        const long long x_ = (long long)(a), y_ = (long long)(b);                                               \
        if (x_ != y_) { printf("FAIL %s:%d  %s = %lld, expected %lld\n", __FILE__, __LINE__, #a, x_, y_); failures++; } \
    } while (0)

int main() {
    using vlq::placement_rank;
    const int nlist = 64;
    // rank = a permutation that is not the identity; part = rank * 8 / nlist, as the handle builds it
    std::vector<int> rank(nlist);
    std::vector<uint8_t> part(nlist);
    for (int i = 0; i < nlist; i++) { rank[i] = (i * 37 + 11) % nlist; part[i] = (uint8_t)(rank[i] * 8 / nlist); }
    auto list_of_rank = [&](int r) { for (int i = 0; i < nlist; i++) if (rank[i] == r) return (int64_t)i; return (int64_t)-1; };
    auto key = [&](const std::vector<int64_t>& k, bool with_part = true, bool with_rank = true) {
        std::vector<int64_t> heap(k);      // exactly nprobe elements
        return placement_rank(heap.data(), (int)heap.size(), nlist, with_rank ? rank.data() : nullptr,
                              with_rank && with_part ? part.data() : nullptr);
    };
    // a clear majority: the nearest list lies in partition 0, five of eight probes in partition 3 (ranks 24..31)
    {
        std::vector<int64_t> k = {list_of_rank(2), list_of_rank(30), list_of_rank(25), list_of_rank(50), list_of_rank(27),
                                  list_of_rank(24), list_of_rank(31), list_of_rank(9)};
        CHECK_EQ(key(k), 30);                       // the nearest probe of partition 3
        CHECK_EQ(key(k, false), 2);                 // no list_part: the rank of the nearest list, the key as it was
        CHECK_EQ(key(k, false, false), k[0]);       // no list_rank: its id
    }
    // a tie goes to the partition of the nearest tied probe: 2 + 2 + 1, partition 5 (ranks 40..47) comes first
    {
        std::vector<int64_t> k = {list_of_rank(60), list_of_rank(41), list_of_rank(8), list_of_rank(9), list_of_rank(47)};
        CHECK_EQ(key(k), 41);
        std::vector<int64_t> k2 = {list_of_rank(8), list_of_rank(41), list_of_rank(60), list_of_rank(9), list_of_rank(47)};
        CHECK_EQ(key(k2), 8);
        std::vector<int64_t> one = {list_of_rank(33)};
        CHECK_EQ(key(one), 33);
    }
    // invalid keys: a query whose nearest key is invalid goes to the last bin, with or without the vote; invalid keys behind a
    // valid one do not vote
    {
        std::vector<int64_t> all = {-1, -1, -1, -1};
        CHECK_EQ(key(all), vlq::kPlacementInvalid);
        CHECK_EQ(key(all, false), vlq::kPlacementInvalid);
        CHECK_EQ(key(all, false, false), vlq::kPlacementInvalid);
        std::vector<int64_t> first = {-1, list_of_rank(3), list_of_rank(4)};
        CHECK_EQ(key(first), vlq::kPlacementInvalid);
        std::vector<int64_t> range = {nlist, 1, 2};
        CHECK_EQ(key(range), vlq::kPlacementInvalid);
        std::vector<int64_t> holes = {list_of_rank(20), -1, (int64_t)nlist + 5, list_of_rank(57), -1, list_of_rank(58), -1};
        CHECK_EQ(key(holes), 57);
        CHECK_EQ(vlq::placement_bin(vlq::kPlacementInvalid, 0, nlist + 1), nlist);
        CHECK_EQ(vlq::placement_bin(57, 0, nlist + 1), 57);
        CHECK_EQ(vlq::placement_bin(57, 2, 17), 14);
    }
    // only the nearest 64 probes vote (one per lane in the wave form): 64 probes of partition 0/1 first, 100 of partition 7 behind
    {
        std::vector<int64_t> k;
        for (int i = 0; i < 64; i++) k.push_back(list_of_rank(i % 16));
        for (int i = 0; i < 100; i++) k.push_back(list_of_rank(56 + i % 8));
        CHECK_EQ(key(k), 0);
    }
    // without list_part the key equals the old one for every list
    for (int i = 0; i < nlist; i++) {
        std::vector<int64_t> k = {i, (i + 1) % nlist, (i + 2) % nlist};
        CHECK_EQ(key(k, false), rank[i]);
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("all ok\n");
    return 0;
}
