// The distance of one stored IVFFlat row kept as float16 (GpuIndexIVFFlatConfig::useFloat16IVFStorage, gpu/impl/IVFFlatScan.cu:
// "even if the input data is half, we perform all math in float32"), as a part the k-NN scan (scan_flat16.hip) and the range
// scan (scan_range_flat16.hip) both include.  A stored component is half(x), round to nearest even; the query stays fp32; the
// distance is fvec_L2sqr / fvec_inner_product of (q, float(h)) in the operation order of sse_order.cuh -- four accumulators
// over d in steps of 4, sub / mul / add never fused, the inner product's `+ 0.f` tail, (s0 + s1) + (s2 + s3).  half -> float is
// exact (subnormal halves included), so an f16 index over x gives the bits of the fp32 index over float(half(x)).
//
// Read path kFlatReadTile128 (d % 8 == 0: rows are 16-byte aligned).  A 128-byte piece of a row holds 64 components.  Eight
// neighbouring lanes fetch one row's piece with one dwordx4 each, eight instructions fetch the pieces of the wave's 64 rows
// (each instruction covers 8 rows x 128 B: whole lines), and the 64 x 128 B tile is turned through the wave's own LDS area,
// rows kFlatTileStride floats (144 B) apart: lane l then reads row l with eight ds_read_b128 of eight halves each, converts
// them and feeds the four chains against the query, which sits in LDS as fp32 and is read by broadcast (two b128 per eight
// components).  The next tile -- the next 128 bytes of the same rows, or the first piece of the wave's next 64 rows, clamped
// to the list -- is in flight while the current one is consumed.  d <= 64 is a single piece: the chunk loop runs once.
// Read path kFlatReadRow (d % 8 != 0): every lane walks its own row, by 8-byte loads when d % 4 == 0 (rows are 8-byte
// aligned), by 2-byte loads through l2sqr_sse_order / ip_sse_order otherwise.
//
// flat16_dist_tile128 restates flat_dist.cuh's flat_dist_tile128 (and with it the body of scan_flat_kernel) with a converting
// reader, and flat16_meta_fill restates scan_flat.hip's flat_meta_fill and scan_range_flat.hip's range_meta_fill; those files
// were to stay as they are.  Only the tests keep the copies equal: AN EDIT TO THE OPERATION ORDER, THE CLAMPS OR THE KEY RULES
// IN ONE MUST BE MIRRORED IN THE OTHERS (flat_dist.cuh carries the same warning for the fp32 pair).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flat_plan.h"
#include "kernels.h"
#include "scan16_common.cuh"
#include "sse_order.cuh"

namespace vlq {

typedef float f16_v4f __attribute__((ext_vector_type(4)));
typedef uint32_t f16_v4u __attribute__((ext_vector_type(4)));       // 16 bytes of a row: eight halves, one dwordx4 / ds b128
typedef _Float16 f16_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16_h4 __attribute__((ext_vector_type(4)));
struct Flat16Tile { f16_v4u r[8]; };

constexpr int kFlat16Chunk = 64;          // halves of a row per tile (128 bytes)

// four components of the four chains: s_l += (x_l - y_l)^2 or x_l * y_l, never fused
template <bool IP>
__device__ __forceinline__ void flat16_acc4(float& s0, float& s1, float& s2, float& s3, f16_v4f x, float y0, float y1, float y2, float y3) {
    if constexpr (IP) {
        s0 = __fadd_rn(s0, __fmul_rn(x.x, y0));
        s1 = __fadd_rn(s1, __fmul_rn(x.y, y1));
        s2 = __fadd_rn(s2, __fmul_rn(x.z, y2));
        s3 = __fadd_rn(s3, __fmul_rn(x.w, y3));
    } else {
        const float a0 = __fsub_rn(x.x, y0), a1 = __fsub_rn(x.y, y1), a2 = __fsub_rn(x.z, y2), a3 = __fsub_rn(x.w, y3);
        s0 = __fadd_rn(s0, __fmul_rn(a0, a0));
        s1 = __fadd_rn(s1, __fmul_rn(a1, a1));
        s2 = __fadd_rn(s2, __fmul_rn(a2, a2));
        s3 = __fadd_rn(s3, __fmul_rn(a3, a3));
    }
}

// the end of both reductions when d % 4 == 0: fvec_inner_product adds its tail term whatever d is (utils.cpp:527-530),
// fvec_L2sqr has none
template <bool IP>
__device__ __forceinline__ float flat16_finish(float s0, float s1, float s2, float s3) {
    if constexpr (IP) { s0 = __fadd_rn(s0, 0.f); s1 = __fadd_rn(s1, 0.f); s2 = __fadd_rn(s2, 0.f); s3 = __fadd_rn(s3, 0.f); }
    return __fadd_rn(__fadd_rn(s0, s1), __fadd_rn(s2, s3));
}

// tile (rows j0 .. j0+63, halves c0 .. c0+63) of the list at `base`: instruction i fetches rows 8i .. 8i+7, lane l the piece
// l % 8 of row 8i + l / 8.  Rows are clamped to the list (len >= 1) and pieces to the row (d >= 8), so nothing outside the
// list is touched; what a clamped lane fetches is never read back.
__device__ __forceinline__ Flat16Tile flat16_tile_fetch(const _Float16* __restrict__ base, uint32_t j0, int c0, uint32_t len, int d, int lane) {
    Flat16Tile t;
    const int col = min(c0 + (lane & 7) * 8, d - 8);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t row = min(j0 + (uint32_t)(i * 8 + (lane >> 3)), len - 1);
        t.r[i] = *reinterpret_cast<const f16_v4u*>(base + (size_t)row * d + col);
    }
    return t;
}

// Read path kFlatReadTile128: the distance of row j0 + lane to the query `sq` (LDS, fp32).  `cur` holds the first tile of rows
// j0 .. j0+63 on entry and the first tile of rows j_next .. j_next+63 on return; `tile` is the wave's own
// [64][kFlatTileStride] floats of LDS.  The value of a lane whose row lies behind the list is that of a clamped row: the
// caller masks it.
template <bool IP>
__device__ __forceinline__ float flat16_dist_tile128(const _Float16* __restrict__ base, uint32_t j0, uint32_t j_next, uint32_t len, int d,
                                                     int lane, float* tile, const float* sq, Flat16Tile& cur) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int c0 = 0; c0 < d; c0 += kFlat16Chunk) {
        const bool last = c0 + kFlat16Chunk >= d;
        const Flat16Tile nxt = flat16_tile_fetch(base, last ? j_next : j0, last ? 0 : c0 + kFlat16Chunk, len, d, lane);
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

// Read path kFlatReadRow: the lane walks its own row y.
template <bool IP>
__device__ __forceinline__ float flat16_dist_row(const float* sq, const _Float16* __restrict__ y, int d) {
    if (d % 4 == 0) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int i = 0; i < d; i += 4) {
            const f16_h4 h = *reinterpret_cast<const f16_h4*>(y + i);
            flat16_acc4<IP>(s0, s1, s2, s3, *reinterpret_cast<const f16_v4f*>(sq + i), (float)h[0], (float)h[1], (float)h[2], (float)h[3]);
        }
        return flat16_finish<IP>(s0, s1, s2, s3);
    }
    if constexpr (IP) return ip_sse_order([&](int i) { return sq[i]; }, [&](int i) { return (float)y[i]; }, d);
    else return l2sqr_sse_order([&](int i) { return sq[i]; }, [&](int i) { return (float)y[i]; }, d);
}

// The probes of query q into LDS (scan_flat.hip's flat_meta_fill and scan_range_flat.hip's range_meta_fill).  A key outside
// 0 .. nlist-1 is never walked.  k-NN (RANGE = false): a key < 0 is skipped, a key >= nlist is the bad key; *nvisit = this
// thread's keys in 0 .. nlist-1, empty lists included (IndexIVFFlatStats::nlist).  Range: every key outside is the bad key.
template <bool RANGE>
__device__ __forceinline__ bool flat16_meta_fill(const ScanArgs& a, int64_t q, ProbeMeta& pm, int t0, int nthr, int* nvisit) {
    const int64_t* kq = a.keys + q * a.nprobe;
    bool badkey = false;
    int nv = 0;
    for (int p = t0; p < a.nprobe; p += nthr) {
        const int64_t key = kq[p];
        const bool live = key >= 0 && key < a.nlist;
        if (RANGE ? !live : key >= a.nlist) badkey = true;
        int64_t off = 0, len = 0;
        if (live) { off = a.list_off[key]; len = a.list_len ? a.list_len[key] : a.list_off[key + 1] - off; nv++; }
        pm.poff[p] = off;
        pm.plen[p] = (uint32_t)len;
        pm.pkey[p] = (live && len > 0) ? (int32_t)key : -1;
        if (!RANGE) pm.pd0[p] = 0.f;
    }
    *nvisit = nv;
    return badkey;
}

}  // namespace vlq
