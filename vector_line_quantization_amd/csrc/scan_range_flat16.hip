// Range scan of IndexIVFFlat (IndexIVFFlat::range_search, IndexIVF.cpp:401-449) over float16 lists: scan_range_flat.hip's two
// passes -- count (ballot + popcount per 64-row group, the query's total to lims[q + 1]) and fill (hit r of query q in scan
// order to slot lims[q] + r; the four waves exchange their counts through LDS once per 256-row trip, two sets used in turn;
// no atomics) -- over the row reader and distance body of flat16_dist.cuh, which the k-NN scan (scan_flat16.hip) shares: the
// distances are that scan's bit for bit, and those of the fp32 range scan over float(half(x)).  A hit is dis < radius (L2) or
// ip > radius (inner product), strict; a key < 0 or >= nlist raises the bad-key flag and is not walked.  Both passes run every
// wave through every trip of every visited list, so that the barriers of the fill pass meet.
#include "flat16_dist.cuh"
#include "range_plan.h"
#include "scan_common.cuh"

namespace vlq {

template <bool IP, bool TILE, bool FILL>
__global__ __launch_bounds__(256) void range_flat16_kernel(ScanArgs a, RangeLayout lay, float radius, int64_t* lims) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    uint32_t* xch = reinterpret_cast<uint32_t*>(smraw + lay.xch);                  // [2][4] hit counts of a trip's four groups
    ProbeMeta pm;
    pm.carve(smraw + lay.meta, a.nprobe);
    float* sq = reinterpret_cast<float*>(smraw + lay.sq);                          // [d] the query, fp32

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t q = blockIdx.x;
    const int d = a.d;
    const float* qv = a.queries + q * d;
    const _Float16* vecs = reinterpret_cast<const _Float16*>(a.codes);
    float* tile = reinterpret_cast<float*>(smraw) + wave * 64 * kFlatTileStride;   // this wave's [64][kFlatTileStride]

    for (int e = t; e < d; e += 256) sq[e] = qv[e];
    int nvisit = 0;
    const bool badkey = flat16_meta_fill<true>(a, q, pm, t, 256, &nvisit);
    if (!FILL && badkey) *a.bad_key = 1;               // (every thread looked at its own probes)
    __syncthreads();

    // count: the hits of this wave's groups.  fill: the slot of the workgroup's next hit, the same value in every wave
    unsigned long long run = FILL ? (unsigned long long)lims[q] : 0ull;
    const unsigned long long end = FILL ? (unsigned long long)lims[q + 1] : 0ull;
    int set = 0;

    for (int p = 0; p < a.nprobe; p++) {
        if (pm.pkey[p] < 0) continue;                  // (workgroup-uniform) an invalid key, an empty list
        const uint32_t len = pm.plen[p];
        const _Float16* base = vecs + (size_t)pm.poff[p] * d;
        const int64_t* idp = a.ids + pm.poff[p];
        Flat16Tile cur = {};
        if (TILE && (uint32_t)wave * 64 < len) cur = flat16_tile_fetch(base, (uint32_t)wave * 64, 0, len, d, lane);
        for (uint32_t t0 = 0; t0 < len; t0 += 256) {   // (workgroup-uniform trips)
            const uint32_t j0 = t0 + (uint32_t)wave * 64, j = j0 + lane;
            float v = 0.f;
            bool hit = false;
            if (j0 < len) {                            // (wave-uniform; once false it stays false in this list)
                if constexpr (TILE) v = flat16_dist_tile128<IP>(base, j0, j0 + 256, len, d, lane, tile, sq, cur);
                else v = flat16_dist_row<IP>(sq, base + (size_t)min(j, len - 1) * d, d);
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

template <bool IP, bool TILE>
static void launch_range16_i(const ScanArgs& a, const RangePlan& P, float radius, int64_t* lims, bool fill, hipStream_t s) {
    if (fill) {
        ensure_dynamic_lds(reinterpret_cast<const void*>(range_flat16_kernel<IP, TILE, true>), P.lay.bytes);
        hipLaunchKernelGGL((range_flat16_kernel<IP, TILE, true>), dim3((unsigned)a.nq), dim3(256), P.lay.bytes, s, a, P.lay, radius, lims);
    } else {
        ensure_dynamic_lds(reinterpret_cast<const void*>(range_flat16_kernel<IP, TILE, false>), P.lay.bytes);
        hipLaunchKernelGGL((range_flat16_kernel<IP, TILE, false>), dim3((unsigned)a.nq), dim3(256), P.lay.bytes, s, a, P.lay, radius, lims);
    }
}

bool launch_range_flat16(const ScanArgs& a, bool inner_product, float radius, int64_t* lims, bool fill, hipStream_t s) {
    if (a.nq <= 0) return true;
    const RangePlan P = plan_flat_range(a.d, a.nprobe, kFlatStoreF16);
    if (!P.ok || a.nq > kRangeMaxQueries) return false;
    const bool tile = P.read == kFlatReadTile128;
    if (inner_product) { if (tile) launch_range16_i<true, true>(a, P, radius, lims, fill, s); else launch_range16_i<true, false>(a, P, radius, lims, fill, s); }
    else { if (tile) launch_range16_i<false, true>(a, P, radius, lims, fill, s); else launch_range16_i<false, false>(a, P, radius, lims, fill, s); }
    return true;
}

}  // namespace vlq
