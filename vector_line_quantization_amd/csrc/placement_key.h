// The key that sorts the queries of a batch onto the XCDs (launch_query_order, scan16.hip; speed only).
//
// XCD x scans the x-th contiguous eighth of the queries sorted by this key, and a table row (term2, 16 KB) is an L2 hit only
// when another workgroup of the same XCD asked for the same list shortly before: which queries share an XCD decides the row
// hit rate before the scan starts.  Up to round 6 the key was the spatial rank of the query's NEAREST
// list, which says little about where its other probes lie.  Now the probes vote:
//     p*  = the one of the eight partitions of neighbouring lists (list_part = list_rank * 8 / nlist, one per XCD) that
//           holds most of the query's nearest min(nprobe, 64) probes; among partitions with equally many, the one that
//           holds the nearest of their probes
//     key = list_rank of the nearest probe that lies in p*
// (tools/placement_keys.py, profiles/r07_placement.txt: 2935 -> 2517 distinct lists per XCD chunk on the headline data.)
// Without list_part the key is the rank of the nearest list, without list_rank its id: the keys of multi-index pages and of
// indexes beyond 2^17 lists are what they were.  A query whose nearest key is invalid (-1 padding, out of range) gets
// kPlacementInvalid, which placement_bin puts into the last bin; invalid keys behind a valid one do not vote.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VLQ_HD __host__ __device__
#else
#define VLQ_HD
#endif

namespace vlq {

constexpr uint32_t kPlacementInvalid = 0xffffffffu;
constexpr int kPlacementVoters = 64;        // probes that vote (one per lane in placement_rank_wave)

VLQ_HD inline uint32_t placement_rank(const int64_t* keys_of_query, int nprobe, int nlist, const int* list_rank,
                                      const uint8_t* list_part) {
    const int64_t k0 = keys_of_query[0];
    if (nprobe < 1 || k0 < 0 || k0 >= nlist) return kPlacementInvalid;
    if (!list_rank) return (uint32_t)k0;
    if (!list_part) return (uint32_t)list_rank[k0];
    // one byte per partition: votes (at most 64) / the nearest voter (descending loop: the lowest index is written last)
    uint64_t cnt = 0, first = 0;
    const int np = nprobe < kPlacementVoters ? nprobe : kPlacementVoters;
#pragma unroll 8
    for (int i = np - 1; i >= 0; i--) {
        const int64_t k = keys_of_query[i];
        if (k < 0 || k >= nlist) continue;
        const int sh = 8 * (list_part[k] & 7);
        cnt += 1ull << sh;
        first = (first & ~(0xffull << sh)) | ((uint64_t)i << sh);
    }
    int best_c = 0, best_f = 0;                 // (probe 0 is valid: some partition has a vote)
    for (int p = 0; p < 8; p++) {
        const int c = (int)((cnt >> (8 * p)) & 0xff), f = (int)((first >> (8 * p)) & 0xff);
        if (c > best_c || (c == best_c && c > 0 && f < best_f)) { best_c = c; best_f = f; }
    }
    return (uint32_t)list_rank[keys_of_query[best_f]];
}

// bin of the counting sort (query_order_bins): the high bits of the key, invalid keys last
VLQ_HD inline int placement_bin(uint32_t rank, int shift, int nbins) {
    return rank == kPlacementInvalid ? nbins - 1 : (int)(rank >> shift);
}

#if defined(__HIPCC__)
// The same key computed by a whole wave that holds probe `lane` of one query in lane `lane` (the coarse stage's last kernel:
// no loop over the probes; probes from 64 on do not vote in either form).  in_row: lane < nprobe.  Every lane returns the key.
__device__ __forceinline__ uint32_t placement_rank_wave(int64_t key, bool in_row, int nlist, const int* __restrict__ list_rank,
                                                        const uint8_t* __restrict__ list_part) {
    const bool ok = in_row && key >= 0 && key < nlist;
    const int k = ok ? (int)key : 0;
    const unsigned long long okm = __ballot(ok);
    if (!(okm & 1ull)) return kPlacementInvalid;
    const int k0 = __builtin_amdgcn_readfirstlane(k);
    if (!list_rank) return (uint32_t)k0;
    if (!list_part) return (uint32_t)list_rank[k0];
    const int part = ok ? (int)(list_part[k] & 7) : 8;
    int best_c = 0, best_f = 0;
#pragma unroll
    for (int p = 0; p < 8; p++) {
        const unsigned long long m = __ballot(part == p);
        const int c = __popcll(m), f = m ? __ffsll((long long)m) - 1 : 64;
        if (c > best_c || (c == best_c && c > 0 && f < best_f)) { best_c = c; best_f = f; }
    }
    return (uint32_t)list_rank[__shfl(k, best_f, 64)];
}
#endif

}  // namespace vlq
