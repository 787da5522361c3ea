// The distance of one stored IVFFlat row, as a part a list scan can include: fvec_L2sqr / fvec_inner_product in the
// reference's operation order (sse_order.cuh; utils.cpp:481-533) over the two read paths of flat_plan.h.  It restates the
// body of scan_flat_kernel (scan_flat.hip) operation for operation -- four accumulators over d in steps of 4, sub / mul /
// add never fused, the inner product's `+ 0.f` tail, (s0 + s1) + (s2 + s3) -- so that a second scan gives the same bits.
// Used by scan_range_flat.hip.  scan_flat.hip still carries its own copy (its code object was to stay as it is), and only the
// fixtures keep the two equal: AN EDIT TO EITHER COPY MUST BE MIRRORED IN THE OTHER, until scan_flat.hip includes this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flat_plan.h"
#include "sse_order.cuh"

namespace vlq {

typedef float flat_v4f __attribute__((ext_vector_type(4)));      // a native 16-byte vector: one dwordx4 / ds b128 access
struct FlatTile { flat_v4f r[8]; };

// tile (rows j0 .. j0+63, floats c0 .. c0+31) of the list at `base`: instruction i fetches rows 8i .. 8i+7, lane l the piece
// l % 8 of row 8i + l / 8.  Rows are clamped to the list (len >= 1) and pieces to the row (d >= 4), so nothing outside the
// list is touched; what a clamped lane fetches is never read back.
__device__ __forceinline__ FlatTile flat_tile_fetch(const float* __restrict__ base, uint32_t j0, int c0, uint32_t len, int d, int lane) {
    FlatTile t;
    const int col = min(c0 + (lane & 7) * 4, d - 4);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t row = min(j0 + (uint32_t)(i * 8 + (lane >> 3)), len - 1);
        t.r[i] = *reinterpret_cast<const flat_v4f*>(base + (size_t)row * d + col);
    }
    return t;
}

// Read path kFlatReadTile128 (d % 4 == 0): the distance of row j0 + lane to the query `sq` (LDS).  `cur` holds the first
// tile of rows j0 .. j0+63 on entry and the first tile of rows j_next .. j_next+63 on return (in flight while the last piece
// is consumed); `tile` is the wave's own [64][kFlatTileStride] LDS area.  The value of a lane whose row lies behind the list
// is that of a clamped row: the caller masks it.
template <bool IP>
__device__ __forceinline__ float flat_dist_tile128(const float* __restrict__ base, uint32_t j0, uint32_t j_next, uint32_t len, int d,
                                                   int lane, float* tile, const float* sq, FlatTile& cur) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int c0 = 0; c0 < d; c0 += kFlatChunk) {
        const bool last = c0 + kFlatChunk >= d;
        const FlatTile nxt = flat_tile_fetch(base, last ? j_next : j0, last ? 0 : c0 + kFlatChunk, len, d, lane);
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

// Read path kFlatReadDword (d % 4 != 0): the lane walks its own row y.
template <bool IP>
__device__ __forceinline__ float flat_dist_dword(const float* sq, const float* __restrict__ y, int d) {
    if constexpr (IP) return ip_sse_order([&](int i) { return sq[i]; }, [&](int i) { return y[i]; }, d);
    else return l2sqr_sse_order([&](int i) { return sq[i]; }, [&](int i) { return y[i]; }, d);
}

}  // namespace vlq
