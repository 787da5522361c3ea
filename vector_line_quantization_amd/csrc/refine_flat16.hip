// IndexRefineFlat over a float16 store (vlq_flat_create_ex with storage = 1): refine_flat.hip's kernel over rows kept as
// half(x).  The query stays fp32 and the per-pair distance is flat16_dist.cuh's -- fvec_L2sqr / fvec_inner_product of
// (q, float(h)) in the reference's operation order --, so an f16 store over x gives the bits of the fp32 store over
// float(half(x)): distances, selected rows and the flag of a label >= ntotal alike.
//
// Mapping (refine_flat_plan.h, kFlatStoreF16): one workgroup per query, the query row in LDS as fp32; trips of 64 candidates,
// one per lane, dealt round-robin to the waves.  d % 8 == 0: a 128-byte piece of a half row holds 64 components; eight
// neighbouring lanes fetch one candidate's piece with one dwordx4 each, the row addresses taken from the wave's 64 labels, and
// the 64 x 128 B tile is turned through the wave's LDS area (the same 144-byte row stride) so that every lane then reads its
// candidate's eight halves with one ds_read_b128 and converts them.  A gathered row costs half the bytes of an fp32 one, a
// chunk loop of d <= 64 runs once.  The next piece's tile is in flight while one is consumed.  d % 8 != 0: every lane walks
// its own row (8-byte loads when d % 4 == 0, 2-byte loads otherwise).  The sort, the bitonic stages, the emit and the flag
// restate refine_flat_kernel's; that file was to stay as it is.  Only the tests keep the copies equal: AN EDIT TO THE KEY RULES
// OR THE STAGES IN ONE MUST BE MIRRORED IN THE OTHER.  No atomics, no scratch memory.
#include <hip/hip_runtime.h>

#include "flat16_dist.cuh"
#include "kernels.h"
#include "wave_topk.cuh"

namespace vlq {

namespace {

// tile (the 64 rows of a trip, halves c0 .. c0+63): instruction i fetches the rows of lanes 8i .. 8i+7, lane l the piece l % 8
// of the row of lane 8i + l / 8 (rows[i], a position < ntotal).  Pieces are clamped to the row (d >= 8); what a clamped lane
// fetches is never read back.
__device__ __forceinline__ Flat16Tile gather16_tile_fetch(const _Float16* __restrict__ base, const uint32_t (&rows)[8], int c0, int d, int lane) {
    Flat16Tile t;
    const int col = min(c0 + (lane & 7) * 8, d - 8);
#pragma unroll
    for (int i = 0; i < 8; i++) t.r[i] = *reinterpret_cast<const f16_v4u*>(base + (size_t)rows[i] * d + col);
    return t;
}

// The distance of the row of this lane's candidate to the query `sq` (LDS): flat16_dist_tile128 (flat16_dist.cuh) operation
// for operation, over gathered rows.  `tile` is the wave's own [64][kFlatTileStride] LDS area.  All 64 lanes take part.
template <bool IP>
__device__ __forceinline__ float gather16_dist_tile128(const _Float16* __restrict__ base, const uint32_t (&rows)[8], int d, int lane, float* tile,
                                                       const float* sq) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    Flat16Tile cur = gather16_tile_fetch(base, rows, 0, d, lane);
    for (int c0 = 0; c0 < d; c0 += kFlat16Chunk) {
        const bool last = c0 + kFlat16Chunk >= d;
        Flat16Tile nxt = cur;
        if (!last) nxt = gather16_tile_fetch(base, rows, c0 + kFlat16Chunk, d, lane);
#pragma unroll
        for (int i = 0; i < 8; i++)
            *reinterpret_cast<f16_v4u*>(tile + (i * 8 + (lane >> 3)) * kFlatTileStride + (lane & 7) * 4) = cur.r[i];
        __builtin_amdgcn_wave_barrier();   // (the wave's own area: its LDS accesses complete in order)
        const float* row = tile + lane * kFlatTileStride;
        const float* qc = sq + c0;
        const int npiece = min(kFlat16Chunk, d - c0) >> 3;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            if (c < npiece) {
                const f16_h8 y = *reinterpret_cast<const f16_h8*>(row + 4 * c);
                const f16_v4f x0 = *reinterpret_cast<const f16_v4f*>(qc + 8 * c);
                const f16_v4f x1 = *reinterpret_cast<const f16_v4f*>(qc + 8 * c + 4);
                flat16_acc4<IP>(s0, s1, s2, s3, x0, (float)y[0], (float)y[1], (float)y[2], (float)y[3]);
                flat16_acc4<IP>(s0, s1, s2, s3, x1, (float)y[4], (float)y[5], (float)y[6], (float)y[7]);
            }
        }
        __builtin_amdgcn_wave_barrier();
        cur = nxt;
    }
    return flat16_finish<IP>(s0, s1, s2, s3);
}

struct RefineFlat16Launch {
    RefineFlatArgs a;
    int trips, slots, off_keys, off_labels, off_sq;
};

template <bool IP, bool TILE, bool SELECT>
__global__ __launch_bounds__(64 * kRefineFlatMaxWaves) void refine_flat16_kernel(RefineFlat16Launch p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RefineFlatArgs& a = p.a;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    const int64_t q = blockIdx.x;
    const int d = a.d, kb = a.k_base;
    const _Float16* xh = reinterpret_cast<const _Float16*>(a.xb);       // the stored rows: d halves each
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
                dis = gather16_dist_tile128<IP>(xh, rows, d, lane, tile, sq);
            } else {
                if (live) dis = flat16_dist_row<IP>(sq, xh + (size_t)lab * d, d);
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
void launch_refine_flat16_t(const RefineFlat16Launch& p, int waves, size_t lds, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(&refine_flat16_kernel<IP, TILE, SELECT>), lds);     // (a wide query row passes 64 KB)
    hipLaunchKernelGGL((refine_flat16_kernel<IP, TILE, SELECT>), dim3((unsigned)p.a.nq), dim3(64 * waves), lds, s, p);
}

template <bool IP>
void launch_refine_flat16_m(const RefineFlat16Launch& p, bool tile, bool select, int waves, size_t lds, hipStream_t s) {
    if (tile) { if (select) launch_refine_flat16_t<IP, true, true>(p, waves, lds, s); else launch_refine_flat16_t<IP, true, false>(p, waves, lds, s); }
    else      { if (select) launch_refine_flat16_t<IP, false, true>(p, waves, lds, s); else launch_refine_flat16_t<IP, false, false>(p, waves, lds, s); }
}

}  // namespace

bool launch_refine_flat16(const RefineFlatArgs& a, const RefineFlatPlan& P, bool select, hipStream_t s) {
    if (!P.ok || a.nq > P.page) return false;
    if (a.nq <= 0) return true;
    RefineFlat16Launch p;
    p.a = a;
    p.trips = P.trips; p.slots = P.slots;
    p.off_keys = P.lay.keys; p.off_labels = P.lay.labels; p.off_sq = P.lay.sq;
    const bool tile = P.read == kFlatReadTile128;
    if (a.ip) launch_refine_flat16_m<true>(p, tile, select, P.waves, P.lds, s);
    else launch_refine_flat16_m<false>(p, tile, select, P.waves, P.lds, s);
    return true;
}

}  // namespace vlq
