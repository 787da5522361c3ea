// Range scan of IndexIVFFlat (IndexIVFFlat::range_search, IndexIVF.cpp:401-449): every stored vector of the probed lists whose
//   L2            fvec_L2sqr(q, y, d)          <  radius   (:433-436)
//   inner product fvec_inner_product(q, y, d)  >  radius   (:438-441)
// is a hit (strict; a NaN on either side is none), and the hits of a query come out in scan order: the probes in the order
// given, the rows of a list in stored order -- what the reference's threads, each walking every query, all write.  A key < 0
// or >= nlist aborts the reference's call (:421-425): the bad-key flag.  Distances are those of the k-NN scan bit for bit
// (flat_dist.cuh: the reference's SSE operation order over the read paths of flat_plan.h).
//
// The walk is scan_flat_kernel's: one workgroup of four waves per query, the query in LDS, wave w takes rows w*64 .. w*64+63 of
// every 256 (a trip).  The output is variable-length and ordered, so there are two passes over the same code:
//   count (FILL = false)  ballot + popcount per 64-row group; the query's total goes to lims[q + 1], which the host sums in
//                         place into the limits (RangeSearchResult::lims) and reads to size D and I exactly.
//   fill  (FILL = true)   the distances again; hit r of query q in scan order goes to slot lims[q] + r.  Within a group the slot
//                         is popcount(ballot & lanes below); the group's first slot is the workgroup's running count plus the
//                         counts of the waves in front of it in the same trip, which the four waves exchange through LDS once
//                         per trip (two sets of counts used in turn: one barrier per trip).  No atomics, no sort: the order comes
//                         out of the addressing.
// Both passes run every wave through every trip of every visited list, so that the barriers of the fill pass meet; rows,
// clamps and validity are the same expressions in both.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "flat_dist.cuh"
#include "kernels.h"
#include "range_plan.h"
#include "scan_common.cuh"
#include "scan16_common.cuh"

namespace vlq {

namespace {

// The probes of query q into LDS.  Returns whether this thread saw a key outside 0 .. nlist-1; such a probe is not walked.
__device__ __forceinline__ bool range_meta_fill(const ScanArgs& a, int64_t q, ProbeMeta& pm, int t0, int nthr) {
    const int64_t* kq = a.keys + q * a.nprobe;
    bool badkey = false;
    for (int p = t0; p < a.nprobe; p += nthr) {
        const int64_t key = kq[p];
        const bool live = key >= 0 && key < a.nlist;
        if (!live) badkey = true;
        int64_t off = 0, len = 0;
        if (live) { off = a.list_off[key]; len = a.list_len ? a.list_len[key] : a.list_off[key + 1] - off; }
        pm.poff[p] = off;
        pm.plen[p] = (uint32_t)len;
        pm.pkey[p] = (live && len > 0) ? (int32_t)key : -1;
    }
    return badkey;
}

}  // namespace

template <bool IP, bool VEC4, bool FILL>
__global__ __launch_bounds__(256) void range_flat_kernel(ScanArgs a, RangeLayout lay, float radius, int64_t* lims) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    uint32_t* xch = reinterpret_cast<uint32_t*>(smraw + lay.xch);                  // [2][4] hit counts of a trip's four groups
    ProbeMeta pm;
    pm.carve(smraw + lay.meta, a.nprobe);
    float* sq = reinterpret_cast<float*>(smraw + lay.sq);                          // [d] the query

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t q = blockIdx.x;
    const int d = a.d;
    const float* qv = a.queries + q * d;
    const float* vecs = reinterpret_cast<const float*>(a.codes);
    float* tile = reinterpret_cast<float*>(smraw) + wave * 64 * kFlatTileStride;   // this wave's [64][kFlatTileStride]

    for (int e = t; e < d; e += 256) sq[e] = qv[e];
    const bool badkey = range_meta_fill(a, q, pm, t, 256);
    if (!FILL && badkey) *a.bad_key = 1;               // (every thread looked at its own probes)
    __syncthreads();

    // count: the hits of this wave's groups.  fill: the slot of the workgroup's next hit, the same value in every wave
    unsigned long long run = FILL ? (unsigned long long)lims[q] : 0ull;
    const unsigned long long end = FILL ? (unsigned long long)lims[q + 1] : 0ull;
    int set = 0;

    for (int p = 0; p < a.nprobe; p++) {
        if (pm.pkey[p] < 0) continue;                  // (workgroup-uniform) an invalid key, an empty list
        const uint32_t len = pm.plen[p];
        const float* base = vecs + (size_t)pm.poff[p] * d;
        const int64_t* idp = a.ids + pm.poff[p];
        FlatTile cur = {};
        if (VEC4 && (uint32_t)wave * 64 < len) cur = flat_tile_fetch(base, (uint32_t)wave * 64, 0, len, d, lane);
        for (uint32_t t0 = 0; t0 < len; t0 += 256) {   // (workgroup-uniform trips)
            const uint32_t j0 = t0 + (uint32_t)wave * 64, j = j0 + lane;
            float v = 0.f;
            bool hit = false;
            if (j0 < len) {                            // (wave-uniform; once false it stays false in this list)
                if constexpr (VEC4) v = flat_dist_tile128<IP>(base, j0, j0 + 256, len, d, lane, tile, sq, cur);
                else v = flat_dist_dword<IP>(sq, base + (size_t)min(j, len - 1) * d, d);
                hit = j < len && (IP ? v > radius : v < radius);
            }
            const unsigned long long mask = __ballot(hit);
            const uint32_t cnt = (uint32_t)__popcll(mask);
            if constexpr (!FILL) {
                run += cnt;
            } else {
                if (lane == 0) xch[set * 4 + wave] = cnt;
                __syncthreads();
                const uint32_t c0 = xch[set * 4 + 0], c1 = xch[set * 4 + 1], c2 = xch[set * 4 + 2], c3 = xch[set * 4 + 3];
                set ^= 1;
                const unsigned long long slot = run + (wave > 0 ? c0 : 0u) + (wave > 1 ? c1 : 0u) + (wave > 2 ? c2 : 0u) +
                                                (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
                run += (unsigned long long)c0 + c1 + c2 + c3;
                if (hit && slot < end) {               // (slot < end always: the count pass saw the same hits)
                    a.D[slot] = v;
                    a.I[slot] = idp[j];
                }
            }
        }
    }

    if constexpr (!FILL) {
        unsigned long long* w = reinterpret_cast<unsigned long long*>(xch);       // (32 bytes the count pass has not used so far)
        if (lane == 0) w[wave] = run;
        __syncthreads();
        if (t == 0) lims[q + 1] = (int64_t)(w[0] + w[1] + w[2] + w[3]);
    }
}

template <bool IP, bool VEC4>
static void launch_range_i(const ScanArgs& a, const RangePlan& P, float radius, int64_t* lims, bool fill, hipStream_t s) {
    if (fill) {
        ensure_dynamic_lds(reinterpret_cast<const void*>(range_flat_kernel<IP, VEC4, true>), P.lay.bytes);
        hipLaunchKernelGGL((range_flat_kernel<IP, VEC4, true>), dim3((unsigned)a.nq), dim3(256), P.lay.bytes, s, a, P.lay, radius, lims);
    } else {
        ensure_dynamic_lds(reinterpret_cast<const void*>(range_flat_kernel<IP, VEC4, false>), P.lay.bytes);
        hipLaunchKernelGGL((range_flat_kernel<IP, VEC4, false>), dim3((unsigned)a.nq), dim3(256), P.lay.bytes, s, a, P.lay, radius, lims);
    }
}

bool launch_range_flat(const ScanArgs& a, bool inner_product, float radius, int64_t* lims, bool fill, hipStream_t s) {
    if (a.nq <= 0) return true;
    const RangePlan P = plan_flat_range(a.d, a.nprobe);
    if (!P.ok || a.nq > kRangeMaxQueries) return false;
    const bool vec4 = P.read == kFlatReadTile128;
    if (inner_product) { if (vec4) launch_range_i<true, true>(a, P, radius, lims, fill, s); else launch_range_i<true, false>(a, P, radius, lims, fill, s); }
    else { if (vec4) launch_range_i<false, true>(a, P, radius, lims, fill, s); else launch_range_i<false, false>(a, P, radius, lims, fill, s); }
    return true;
}

hipError_t range_lims_scan(int64_t* v, int64_t n, void* tmp, size_t* tmp_bytes, hipStream_t s) {
    return rocprim::inclusive_scan(tmp, *tmp_bytes, v, v, (size_t)n, rocprim::plus<int64_t>(), s);
}

}  // namespace vlq
