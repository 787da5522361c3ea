// IndexRefineFlat on the device: IndexFlat::compute_distance_subset (IndexFlat.cpp:73-93; fvec_L2sqr_by_idx /
// fvec_inner_products_by_idx, utils.cpp:974-1012) and the selection of IndexRefineFlat::search (reorder_2_heaps,
// IndexFlat.cpp:194-213, :245-260).
//
// Per shortlist entry (a row position of the flat store, < 0 = skip), the distance is fvec_L2sqr / fvec_inner_product of the
// query and the stored row in the reference's operation order (flat_dist.cuh: four accumulators over d in steps of 4, sub /
// mul / add never fused, the scalar tail, the inner product's `+ 0.f`, (s0 + s1) + (s2 + s3)); a skipped entry keeps the
// distance it came in with.  There is no BLAS branch on this path: every distance has the same bits at every batch size.
// The selection is a total order on 64-bit keys (order-preserving image of the distance << 32 | shortlist position; inner
// product: the image complemented, so that larger comes first and a lower position first among equals): the k first keys of
// the sorted row are the reference's heap result, up to the order of exactly equal distances.
//
// Mapping (refine_flat_plan.h): one workgroup per query, the query row in LDS.  A trip is 64 candidates, one per lane; the
// trips are dealt round-robin to the waves.  d % 4 == 0: the candidates' rows cross from memory as the IVFFlat scan's list rows
// do -- eight neighbouring lanes fetch one row's 128-byte piece, a wave instruction 8 rows x 128 B -- with the row addresses
// taken from the wave's 64 labels, and the 64 x 128 B tile is turned through the wave's LDS area so that every lane then owns
// its candidate's row.  The next piece's tile is in flight while one is consumed.  d % 4 != 0: every lane walks its own row.
// A wave sorts each trip's keys in registers (odd trips descending); the remaining bitonic stages of the row run in LDS over
// the whole workgroup.  No atomics, no scratch memory.
#include <hip/hip_runtime.h>

#include "flat_dist.cuh"
#include "kernels.h"
#include "wave_topk.cuh"

namespace vlq {

namespace {

// tile (the 64 rows of a trip, floats c0 .. c0+31): instruction i fetches the rows of lanes 8i .. 8i+7, lane l the piece l % 8
// of the row of lane 8i + l / 8 (rows[i], a position < ntotal).  Pieces are clamped to the row (d >= 4); what a clamped lane
// fetches is never read back.
__device__ __forceinline__ FlatTile gather_tile_fetch(const float* __restrict__ base, const uint32_t (&rows)[8], int c0, int d, int lane) {
    FlatTile t;
    const int col = min(c0 + (lane & 7) * 4, d - 4);
#pragma unroll
    for (int i = 0; i < 8; i++) t.r[i] = *reinterpret_cast<const flat_v4f*>(base + (size_t)rows[i] * d + col);
    return t;
}

// The distance of the row of this lane's candidate to the query `sq` (LDS): flat_dist_tile128 (flat_dist.cuh) operation for
// operation, over gathered rows.  `tile` is the wave's own [64][kFlatTileStride] LDS area.  All 64 lanes take part.
template <bool IP>
__device__ __forceinline__ float gather_dist_tile128(const float* __restrict__ base, const uint32_t (&rows)[8], int d, int lane, float* tile,
                                                     const float* sq) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    FlatTile cur = gather_tile_fetch(base, rows, 0, d, lane);
    for (int c0 = 0; c0 < d; c0 += kFlatChunk) {
        const bool last = c0 + kFlatChunk >= d;
        FlatTile nxt = cur;
        if (!last) nxt = gather_tile_fetch(base, rows, c0 + kFlatChunk, d, lane);
#pragma unroll
        for (int i = 0; i < 8; i++)
            *reinterpret_cast<flat_v4f*>(tile + (i * 8 + (lane >> 3)) * kFlatTileStride + (lane & 7) * 4) = cur.r[i];
        __builtin_amdgcn_wave_barrier();   // (the wave's own area: its LDS accesses complete in order)
        const float* row = tile + lane * kFlatTileStride;
        const float* qc = sq + c0;
        const int npiece = min(kFlatChunk, d - c0) >> 2;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            if (c < npiece) {
                const flat_v4f y = *reinterpret_cast<const flat_v4f*>(row + 4 * c);
                const flat_v4f x = *reinterpret_cast<const flat_v4f*>(qc + 4 * c);
                if constexpr (IP) {
                    s0 = __fadd_rn(s0, __fmul_rn(x.x, y.x));
                    s1 = __fadd_rn(s1, __fmul_rn(x.y, y.y));
                    s2 = __fadd_rn(s2, __fmul_rn(x.z, y.z));
                    s3 = __fadd_rn(s3, __fmul_rn(x.w, y.w));
                } else {
                    const float a0 = __fsub_rn(x.x, y.x), a1 = __fsub_rn(x.y, y.y);
                    const float a2 = __fsub_rn(x.z, y.z), a3 = __fsub_rn(x.w, y.w);
                    s0 = __fadd_rn(s0, __fmul_rn(a0, a0));
                    s1 = __fadd_rn(s1, __fmul_rn(a1, a1));
                    s2 = __fadd_rn(s2, __fmul_rn(a2, a2));
                    s3 = __fadd_rn(s3, __fmul_rn(a3, a3));
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        cur = nxt;
    }
    if constexpr (IP) {     // the tail term of fvec_inner_product is added whatever d is (utils.cpp:527-530)
        s0 = __fadd_rn(s0, 0.f); s1 = __fadd_rn(s1, 0.f); s2 = __fadd_rn(s2, 0.f); s3 = __fadd_rn(s3, 0.f);
    }
    return __fadd_rn(__fadd_rn(s0, s1), __fadd_rn(s2, s3));
}

struct RefineFlatLaunch {
    RefineFlatArgs a;
    int trips, slots, off_keys, off_labels, off_sq;
};

template <bool IP, bool TILE, bool SELECT>
__global__ __launch_bounds__(64 * kRefineFlatMaxWaves) void refine_flat_kernel(RefineFlatLaunch p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RefineFlatArgs& a = p.a;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    const int64_t q = blockIdx.x;
    const int d = a.d, kb = a.k_base;
    float* tile = reinterpret_cast<float*>(smem) + wave * (kRefineFlatTrip * kFlatTileStride);
    u64* keys = reinterpret_cast<u64*>(smem + p.off_keys);             // [slots]
    int64_t* labs = reinterpret_cast<int64_t*>(smem + p.off_labels);   // [slots]
    float* sq = reinterpret_cast<float*>(smem + p.off_sq);             // [d]
    for (int c = threadIdx.x; c < d; c += blockDim.x) sq[c] = a.x[q * d + c];
    __syncthreads();

    const int64_t* lab_row = a.labels + q * kb;
    // select: every 64 keys of the sorted row are written, the ones behind the shortlist as kMaxKey
    const int nchunk = SELECT ? p.slots / kRefineFlatTrip : p.trips;
    for (int t = wave; t < nchunk; t += nwaves) {
        const int j = t * kRefineFlatTrip + lane;
        const bool in = j < kb;
        const int64_t lab = in ? lab_row[j] : -1;
        bool live = lab >= 0;                          // IndexFlat.cpp / utils.cpp:984, :1004: `if (idsj[j] < 0) continue`
        if (live && lab >= a.ntotal) {                 // the reference asserts (IndexFlat.cpp:240-242): never dereferenced
            *a.bad = 1;
            live = false;
        }
        float dis = 0.f;
        if (__ballot(live) != 0) {                     // (wave-uniform; a live label implies ntotal >= 1: row 0 exists)
            if constexpr (TILE) {
                const uint32_t mine = live ? (uint32_t)lab : 0u;
                uint32_t rows[8];
#pragma unroll
                for (int i = 0; i < 8; i++) rows[i] = (uint32_t)__shfl((int)mine, i * 8 + (lane >> 3), 64);
                dis = gather_dist_tile128<IP>(a.xb, rows, d, lane, tile, sq);
            } else {
                if (live) dis = flat_dist_dword<IP>(sq, a.xb + (size_t)lab * d, d);
            }
        }
        if constexpr (!SELECT) {
            if (live) a.D[q * kb + j] = dis;
        } else {
            if (in && !live) dis = a.base_D[q * kb + j];
            const uint32_t img = f32_to_ordered(dis);
            u64 key = in ? ((u64)(IP ? ~img : img) << 32) | (uint32_t)j : kMaxKey;
            key = wave_sort64(key, lane);
            if (t & 1) key = lane_reverse_u64(key);    // odd trips descending: pairs of trips are bitonic
            keys[j] = key;
            labs[j] = lab;
        }
    }
    if constexpr (SELECT) {
        __syncthreads();        // (also: every read of base_D / labels is done before a row is written -- they may be D / I)
        for (int size = 2 * kRefineFlatTrip; size <= p.slots; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int i = threadIdx.x; i < p.slots / 2; i += blockDim.x) {
                    const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
                    const int hi = lo + stride;
                    const bool up = (lo & size) == 0;      // (size == slots: lo < slots, ascending)
                    const u64 ka = keys[lo], kb2 = keys[hi];
                    if ((ka > kb2) == up) { keys[lo] = kb2; keys[hi] = ka; }
                }
                __syncthreads();
            }
        }
        for (int e = threadIdx.x; e < a.k; e += blockDim.x) {
            const u64 key = keys[e];                       // (k <= k_base: a shortlist entry, never the padding)
            const uint32_t img = (uint32_t)(key >> 32);
            a.D[q * a.k + e] = ordered_to_f32(IP ? ~img : img);
            a.I[q * a.k + e] = labs[(uint32_t)key];
        }
    }
}

template <bool IP, bool TILE, bool SELECT>
void launch_refine_flat_t(const RefineFlatLaunch& p, int waves, size_t lds, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(&refine_flat_kernel<IP, TILE, SELECT>), lds);     // (a wide query row passes 64 KB)
    hipLaunchKernelGGL((refine_flat_kernel<IP, TILE, SELECT>), dim3((unsigned)p.a.nq), dim3(64 * waves), lds, s, p);
}

template <bool IP>
void launch_refine_flat_m(const RefineFlatLaunch& p, bool tile, bool select, int waves, size_t lds, hipStream_t s) {
    if (tile) { if (select) launch_refine_flat_t<IP, true, true>(p, waves, lds, s); else launch_refine_flat_t<IP, true, false>(p, waves, lds, s); }
    else      { if (select) launch_refine_flat_t<IP, false, true>(p, waves, lds, s); else launch_refine_flat_t<IP, false, false>(p, waves, lds, s); }
}

}  // namespace

bool launch_refine_flat(const RefineFlatArgs& a, const RefineFlatPlan& P, bool select, hipStream_t s) {
    if (!P.ok || a.nq > P.page) return false;
    if (a.nq <= 0) return true;
    RefineFlatLaunch p;
    p.a = a;
    p.trips = P.trips; p.slots = P.slots;
    p.off_keys = P.lay.keys; p.off_labels = P.lay.labels; p.off_sq = P.lay.sq;
    const bool tile = P.read == kFlatReadTile128;
    if (a.ip) launch_refine_flat_m<true>(p, tile, select, P.waves, P.lds, s);
    else launch_refine_flat_m<false>(p, tile, select, P.waves, P.lds, s);
    return true;
}

}  // namespace vlq
