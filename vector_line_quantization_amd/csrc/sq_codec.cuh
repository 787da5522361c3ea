// The scalar-quantizer codec as the scans read it (scan_sq.hip: the IVF list scan; scan_sqflat.hip: the exhaustive scan): the
// 128-byte tile fetch, the range, the decode of one component, one term of the distance and the join of the eight accumulators.
// The operation orders are stated in the header comment of scan_sq.hip; every float operation is on its own, nothing is fused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vlq {

typedef float v4f __attribute__((ext_vector_type(4)));      // a native 16-byte vector: one dwordx4 / ds b128 access
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
struct SqTile { v4u r[8]; };

// tile (rows j0 .. j0+63, bytes c0 .. c0+127) of the list at `base`: instruction i fetches rows 8i .. 8i+7, lane l the piece
// l % 8 of row 8i + l / 8.  Rows are clamped to the list and pieces to the row (code_size >= 16 on this path), so nothing
// outside the list is touched; what a clamped lane fetches is never read back.
__device__ __forceinline__ SqTile sq_tile_load(const uint8_t* __restrict__ base, uint32_t j0, int c0, uint32_t len, int code_size, int lane) {
    SqTile t;
    const int col = min(c0 + (lane & 7) * 16, code_size - 16);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t row = min(j0 + (uint32_t)(i * 8 + (lane >> 3)), len - 1);
        t.r[i] = *reinterpret_cast<const v4u*>(base + (size_t)row * code_size + col);
    }
    return t;
}

// the range of the quantizer as the kernel reads it: per-dimension arrays in LDS, or the two floats of a uniform type
struct SqRange { const float* vmin; const float* vdiff; float vmin0, vdiff0; };

template <int BITS, bool ORDER8>
__device__ __forceinline__ float sq_decode(uint32_t c, float vmin, float vdiff) {
    constexpr float den = BITS == 8 ? 255.f : 15.f;
    const float f = __fadd_rn((float)c, 0.5f);
    const float xi = ORDER8 ? __fmul_rn(f, 1.f / den) : __fdiv_rn(f, den);
    return __fadd_rn(vmin, __fmul_rn(xi, vdiff));
}

template <bool IP>
__device__ __forceinline__ float sq_accumulate(float acc, float y, float rec) {
    if constexpr (IP) return __fadd_rn(acc, __fmul_rn(y, rec));
    const float tmp = __fsub_rn(y, rec);
    return __fadd_rn(acc, __fmul_rn(tmp, tmp));
}

// result_8 (:165-172, :216-224)
template <bool IP>
__device__ __forceinline__ float sq_join8(const float (&a)[8], float accu0) {
    const float lo = __fadd_rn(__fadd_rn(a[0], a[1]), __fadd_rn(a[2], a[3]));
    const float hi = __fadd_rn(__fadd_rn(a[4], a[5]), __fadd_rn(a[6], a[7]));
    if constexpr (IP) return __fadd_rn(__fadd_rn(accu0, lo), hi);
    return __fadd_rn(lo, hi);
}

}  // namespace vlq
