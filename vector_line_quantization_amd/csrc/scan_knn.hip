// Flat exact k-NN: faiss::IndexFlat::search (IndexFlat.cpp:30-56; knn_L2sqr / knn_inner_product, utils.cpp:726-946) on the
// device.  Path, route, row tile, slices and scratch are plan_knn's decision (knn_plan.h).
//   knn_gemm_kernel    the GEMM path fused with the selection (k <= 256).  A workgroup owns ROWS queries and walks the 128-column
//                      tiles of its slice.  Inner products are MfmaTile's (mfma_tile.cuh: the k-ordered f32 MFMA chain of
//                      coarse_dist_kernel), the epilogue is coarse_dist_kernel's expression (x_norm + y_norm) - 2 ip (utils.cpp:884).
//                      The distance tile goes to LDS only; a wave looks at a row's 128 distances, and only if one of them is
//                      below the row's k-th distance (the rule of the coarse stage's tile minima: after the first tiles almost
//                      nothing passes) does it take the row's best keys out of LDS, merge (wave_topk.cuh) and put them back.
//   knn_direct_kernel  nq < 20 && d % 4 == 0: fvec_L2sqr / fvec_inner_product per pair in the reference's order (sse_order.cuh;
//                      the row tiles of flat_dist.cuh).  Every stored vector is fetched once for all queries held in LDS; the
//                      [nq][chunk] distances go to the bounded scratch matrix.
//   knn_select_kernel  one wave per (query, slice of the chunk) over the scratch matrix (the direct path, and the GEMM path with
//                      k > 256, whose matrix is launch_coarse_distances').  The join (join_rows.cuh) folds the slices and the
//                      running row.
// Selection is by the total order (distance, position) everywhere: rows depend on no tiling, slicing, chunking or paging.
// Inner product: keys hold the negated inner product (negation is exact), rows come out descending, padded -FLT_MAX / -1.
#include "kernels.h"
#include "knn_plan.h"
#include "flat_dist.cuh"
#include "join_rows.cuh"
#include "mfma_tile.cuh"
#include "wave_topk.cuh"

#include <algorithm>

namespace vlq {

namespace {

constexpr float kFltMax = 3.402823466e+38f;

template <int KPL>
struct KeyRow { u64 best[KPL]; };

template <int WR, int TI, int TJ, int KPL>
__global__ __launch_bounds__(256) void knn_gemm_kernel(KnnArgs a, int64_t slice_len, int S) {
    typedef MfmaTile<kKnnKC, WR, TI, TJ> Tile;
    constexpr int ROWS = Tile::ROWS, COLS = Tile::COLS, TS = COLS + 1, WC = Tile::WC;
    static_assert(COLS == kKnnColTile, "the plan's column tile");
    constexpr size_t kStage = (size_t)Tile::kLdsFloats * 4, kTile = (size_t)ROWS * TS * 4;
    constexpr size_t kFront = ((kStage > kTile ? kStage : kTile) + 15) / 16 * 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    float* sm = reinterpret_cast<float*>(smraw);                        // the staged tiles, then the distance tile [ROWS][TS]
    u64* best = reinterpret_cast<u64*>(smraw + kFront);                 // [ROWS][64 KPL], ascending
    float* thrs = reinterpret_cast<float*>(best + (size_t)ROWS * 64 * KPL);      // [ROWS] k-th distance of the row so far
    float* qns = thrs + ROWS;                                           // [ROWS] |q|^2
    u64* queue = reinterpret_cast<u64*>(qns + ROWS);                    // [4][64]

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave / WC, wc = wave % WC;
    const int64_t i0 = (int64_t)blockIdx.x * ROWS;
    const int slice = blockIdx.y;
    const int64_t lo = min((int64_t)slice * slice_len, a.ntotal), hi = min(lo + slice_len, a.ntotal);
    const int k = a.k, d = a.d;

    for (int e = t; e < ROWS * 64 * KPL; e += 256) best[e] = kMaxKey;
    for (int r = t; r < ROWS; r += 256) {
        const bool live = i0 + r < a.nq;
        thrs[r] = live ? kFltMax : -__builtin_inff();                   // a row behind nq admits nothing
        qns[r] = (live && !a.ip) ? a.qn[i0 + r] : 0.f;
    }
    __syncthreads();

    // The walk is a sequence of (column tile, k step) steps.  The rows of the step after the current one are fetched into
    // registers before the current one is multiplied, and committed to LDS behind it: the loads fly during the MFMA chain, and
    // those of a tile's first step during the selection of the tile before.
    const bool vec_ok = d % 4 == 0;
    typename Tile::template Frag<ROWS> fa;
    typename Tile::template Frag<COLS> fb;
    if (lo < hi) {
        Tile::template fetch<ROWS>(a.xq, i0, a.nq, d, 0, vec_ok, fa, t);
        Tile::template fetch<COLS>(a.xb, lo, hi, d, 0, vec_ok, fb, t);
    }
    for (int64_t j0 = lo; j0 < hi; j0 += COLS) {
        f32x16 acc[TI][TJ];
#pragma unroll
        for (int ti = 0; ti < TI; ti++)
#pragma unroll
            for (int tj = 0; tj < TJ; tj++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[ti][tj][r] = 0.f;
        for (int k0 = 0; k0 < d; k0 += kKnnKC) {
            Tile::template commit<ROWS>(fa, Tile::lds_a(sm), t);
            Tile::template commit<COLS>(fb, Tile::lds_b(sm), t);
            __syncthreads();
            const bool more_k = k0 + kKnnKC < d;
            const int64_t jn = more_k ? j0 : j0 + COLS;
            if (jn < hi) {
                const int kn = more_k ? k0 + kKnnKC : 0;
                Tile::template fetch<ROWS>(a.xq, i0, a.nq, d, kn, vec_ok, fa, t);
                Tile::template fetch<COLS>(a.xb, jn, hi, d, kn, vec_ok, fb, t);
            }
            Tile::multiply(sm, acc);
            __syncthreads();                            // sm is free: the tile's distances go there next
        }

        // the distance tile, to LDS only; a column behind the slice is FLT_MAX, which nothing admits
        const int h = lane >> 5, cidx = lane & 31;
#pragma unroll
        for (int tj = 0; tj < TJ; tj++) {
            const int coll = (wc * TJ + tj) * 32 + cidx;
            const int64_t col = j0 + coll;
            const bool live = col < hi;
            const float ynv = (live && !a.ip) ? a.yn[col] : 0.f;
#pragma unroll
            for (int ti = 0; ti < TI; ti++) {
#pragma unroll
                for (int reg = 0; reg < 16; reg++) {
                    const int rowl = (wr * TI + ti) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    const float ip = acc[ti][tj][reg];
                    // (x_norm + y_norm) - 2 * ip, utils.cpp:884; inner product: -ip
                    const float dis = a.ip ? flip_sign(ip, 0x80000000u) : __fsub_rn(__fadd_rn(qns[rowl], ynv), __fmul_rn(2.f, ip));
                    sm[rowl * TS + coll] = live ? dis : kFltMax;
                }
            }
        }
        __syncthreads();

        for (int row = wave; row < ROWS; row += 4) {
            const float thr = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(thrs[row])));
            const float v0 = sm[row * TS + lane], v1 = sm[row * TS + 64 + lane];
            if (__ballot(v0 < thr || v1 < thr) == 0) continue;
            // columns arrive in increasing position: the strict test is the heap's (Heap.h:68-79)
            WaveSelect<KPL> sel;
            sel.init(k, queue + wave * 64, lane);
            u64* mine = best + (size_t)row * 64 * KPL;
#pragma unroll
            for (int r = 0; r < KPL; r++) sel.best[r] = mine[r * 64 + lane];
            sel.thr = sel.thr_own = thr;
            sel.offer(v0, (uint32_t)(j0 + lane), true);
            sel.offer(v1, (uint32_t)(j0 + 64 + lane), true);
            sel.flush();
#pragma unroll
            for (int r = 0; r < KPL; r++) mine[r * 64 + lane] = sel.best[r];
            if (lane == 0) thrs[row] = sel.thr_own;
        }
        __syncthreads();                                // the tile area is staged over next
    }

    const uint32_t neg = a.ip ? 0x80000000u : 0u;
    for (int row = wave; row < ROWS; row += 4) {
        const int64_t q = i0 + row;
        if (q >= a.nq) break;
        KeyRow<KPL> kr;
#pragma unroll
        for (int r = 0; r < KPL; r++) kr.best[r] = best[(size_t)row * 64 * KPL + r * 64 + lane];
        if (S > 1) {
            u64* out = a.part + ((size_t)q * S + slice) * k;
#pragma unroll
            for (int r = 0; r < KPL; r++) {
                const int e = r * 64 + lane;
                if (e < k) out[e] = kr.best[r];
            }
        } else {
            pq_emit<KPL>(kr, k, neg, a.D + q * k, a.I + q * k, lane);
        }
    }
}

// out[q][j] = fvec_L2sqr(x_q, y_j) resp. -fvec_inner_product(x_q, y_j) for the QT queries from blockIdx.y * QT on and the rows
// j of the chunk at xb (ncols rows, d % 4 == 0); a wave owns 64 rows, every lane one of them
template <int QT, bool IP>
__global__ __launch_bounds__(256) void knn_direct_kernel(const float* __restrict__ xb, const float* __restrict__ xq, float* __restrict__ out,
                                                         int64_t ld, uint32_t ncols, int nq, int d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    float* sq = reinterpret_cast<float*>(smraw);                                                // [QT][d]
    float* tiles = reinterpret_cast<float*>(smraw + ((size_t)QT * d * 4 + 15) / 16 * 16);       // [4][64][kFlatTileStride]
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int q0 = blockIdx.y * QT;
    const int nqt = min(QT, nq - q0);
    for (int e = t; e < QT * d; e += 256) sq[e] = e < nqt * d ? xq[(size_t)q0 * d + e] : 0.f;
    __syncthreads();
    const uint32_t j0 = (blockIdx.x * 4u + (uint32_t)wave) * 64u;
    if (j0 >= ncols) return;
    float* tile = tiles + wave * 64 * kFlatTileStride;
    float s[QT][4];
#pragma unroll
    for (int q = 0; q < QT; q++) s[q][0] = s[q][1] = s[q][2] = s[q][3] = 0.f;
    FlatTile cur = flat_tile_fetch(xb, j0, 0, ncols, d, lane);
    for (int c0 = 0; c0 < d; c0 += kFlatChunk) {
        const bool last = c0 + kFlatChunk >= d;
        FlatTile nxt = cur;
        if (!last) nxt = flat_tile_fetch(xb, j0, c0 + kFlatChunk, ncols, d, lane);
#pragma unroll
        for (int i = 0; i < 8; i++)
            *reinterpret_cast<flat_v4f*>(tile + (i * 8 + (lane >> 3)) * kFlatTileStride + (lane & 7) * 4) = cur.r[i];
        __builtin_amdgcn_wave_barrier();   // (the wave's own area: its LDS accesses complete in order)
        const float* row = tile + lane * kFlatTileStride;
        const int npiece = min(kFlatChunk, d - c0) >> 2;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            if (c < npiece) {
                const flat_v4f y = *reinterpret_cast<const flat_v4f*>(row + 4 * c);
#pragma unroll
                for (int q = 0; q < QT; q++) {
                    const flat_v4f x = *reinterpret_cast<const flat_v4f*>(sq + q * d + c0 + 4 * c);      // (one address: a broadcast)
                    if constexpr (IP) {
                        s[q][0] = __fadd_rn(s[q][0], __fmul_rn(x.x, y.x));
                        s[q][1] = __fadd_rn(s[q][1], __fmul_rn(x.y, y.y));
                        s[q][2] = __fadd_rn(s[q][2], __fmul_rn(x.z, y.z));
                        s[q][3] = __fadd_rn(s[q][3], __fmul_rn(x.w, y.w));
                    } else {
                        const float a0 = __fsub_rn(x.x, y.x), a1 = __fsub_rn(x.y, y.y);
                        const float a2 = __fsub_rn(x.z, y.z), a3 = __fsub_rn(x.w, y.w);
                        s[q][0] = __fadd_rn(s[q][0], __fmul_rn(a0, a0));
                        s[q][1] = __fadd_rn(s[q][1], __fmul_rn(a1, a1));
                        s[q][2] = __fadd_rn(s[q][2], __fmul_rn(a2, a2));
                        s[q][3] = __fadd_rn(s[q][3], __fmul_rn(a3, a3));
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        cur = nxt;
    }
    const uint32_t j = j0 + (uint32_t)lane;
    if (j >= ncols) return;
#pragma unroll
    for (int q = 0; q < QT; q++) {
        float s0 = s[q][0], s1 = s[q][1], s2 = s[q][2], s3 = s[q][3];
        if constexpr (IP) {     // the tail term of fvec_inner_product is added whatever d is (utils.cpp:527-530)
            s0 = __fadd_rn(s0, 0.f); s1 = __fadd_rn(s1, 0.f); s2 = __fadd_rn(s2, 0.f); s3 = __fadd_rn(s3, 0.f);
        }
        const float v = __fadd_rn(__fadd_rn(s0, s1), __fadd_rn(s2, s3));
        if (q < nqt) out[(size_t)(q0 + q) * ld + j] = IP ? flip_sign(v, 0x80000000u) : v;
    }
}

// the k smallest (scale * mat[q][e], col_base + e) of slice s of the chunk -> slot s + 1 of the query's partial rows
template <int KPL>
__global__ __launch_bounds__(256) void knn_select_kernel(const float* __restrict__ mat, int64_t ld, int64_t nq, int64_t ncols, int64_t col_base,
                                                         int64_t slice_len, int S, float scale, int k, u64* __restrict__ part, int64_t part_stride) {
    __shared__ u64 queue[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    if (item >= nq * S) return;
    const int64_t q = item / S;
    const int s = (int)(item % S);
    const int64_t lo = min((int64_t)s * slice_len, ncols), hi = min(lo + slice_len, ncols);
    WaveSelect<KPL> sel;
    sel.init(k, queue[wave], lane);
    const float* row = mat + (size_t)q * ld;
    for (int64_t e0 = lo; e0 < hi; e0 += 64) {
        const int64_t e = e0 + lane;
        const bool valid = e < hi;
        const float v = valid ? row[e] : 0.f;
        sel.offer(__fmul_rn(v, scale), (uint32_t)(col_base + e), valid);
    }
    sel.flush();
    u64* out = part + (size_t)q * part_stride + (size_t)(s + 1) * k;
#pragma unroll
    for (int r = 0; r < KPL; r++) {
        const int e = r * 64 + lane;
        if (e < k) out[e] = sel.best[r];
    }
}

// ntotal == 0: padded rows (Heap.h:318-321)
__global__ __launch_bounds__(256) void knn_pad_kernel(float* __restrict__ D, int64_t* __restrict__ I, int64_t n, float pad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { D[i] = pad; I[i] = -1; }
}

template <int WR, int TI, int TJ, int KPL>
void launch_gemm_i(const KnnArgs& a, const KnnPlan& P, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(knn_gemm_kernel<WR, TI, TJ, KPL>), P.lds);
    const dim3 grid((unsigned)((a.nq + P.rows - 1) / P.rows), (unsigned)P.S);
    hipLaunchKernelGGL((knn_gemm_kernel<WR, TI, TJ, KPL>), grid, dim3(256), P.lds, s, a, P.slice_len, P.S);
}

template <int QT>
void launch_direct_i(const KnnArgs& a, const KnnPlan& P, const float* xb, int64_t nc, hipStream_t s) {
    const dim3 grid((unsigned)((nc + 255) / 256), (unsigned)((a.nq + QT - 1) / QT));
    if (a.ip) {
        ensure_dynamic_lds(reinterpret_cast<const void*>(knn_direct_kernel<QT, true>), P.lds);
        hipLaunchKernelGGL((knn_direct_kernel<QT, true>), grid, dim3(256), P.lds, s, xb, a.xq, a.matrix, nc, (uint32_t)nc, (int)a.nq, a.d);
    } else {
        ensure_dynamic_lds(reinterpret_cast<const void*>(knn_direct_kernel<QT, false>), P.lds);
        hipLaunchKernelGGL((knn_direct_kernel<QT, false>), grid, dim3(256), P.lds, s, xb, a.xq, a.matrix, nc, (uint32_t)nc, (int)a.nq, a.d);
    }
}

}  // namespace

bool launch_knn(const KnnArgs& a, const KnnPlan& P, hipStream_t s) {
    if (a.nq <= 0) return true;
    if (!P.ok || a.nq > P.page) return false;
    const int k = a.k;
    if (a.ntotal == 0) {
        const int64_t n = a.nq * k;
        hipLaunchKernelGGL(knn_pad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.D, a.I, n, a.ip ? -kFltMax : kFltMax);
        return true;
    }
    const uint32_t neg = a.ip ? 0x80000000u : 0u;
    if (P.route == kKnnFused) {
        if (P.kpl == 1 && P.rows == 128) launch_gemm_i<2, 2, 2, 1>(a, P, s);
        else if (P.kpl == 1 && P.rows == 64) launch_gemm_i<1, 2, 1, 1>(a, P, s);
        else if (P.kpl == 1 && P.rows == 32) launch_gemm_i<1, 1, 1, 1>(a, P, s);
        else if (P.kpl == 4 && P.rows == 32) launch_gemm_i<1, 1, 1, 4>(a, P, s);
        else return false;
        if (P.join) launch_join_rows(P.kpl, a.part, a.nq, P.S, (int64_t)P.S * k, k, neg, a.D, a.I, nullptr, 0, s);
        return true;
    }
    // matrix route: chunk by chunk, the running row in slot 0 of the query's S + 1 partial rows
    const int64_t stride = (int64_t)(P.S + 1) * k;
    const bool direct = P.path == kKnnDirect;
    for (int64_t c0 = 0; c0 < a.ntotal; c0 += P.chunk) {
        const int64_t nc = std::min(P.chunk, a.ntotal - c0);
        const float* xb = a.xb + (size_t)c0 * a.d;
        if (direct) {
            if (P.rows == 19) launch_direct_i<19>(a, P, xb, nc, s);
            else if (P.rows == 4) launch_direct_i<4>(a, P, xb, nc, s);
            else if (P.rows == 1) launch_direct_i<1>(a, P, xb, nc, s);
            else return false;
        } else {
            // knn_L2sqr_blas / knn_inner_product_blas: the coarse stage's distance kernel; zero norms leave -2 ip, halved below
            const float* qn = a.ip ? a.zeros : coarse_norms_fused_ok(a.d) ? nullptr : a.qn;
            launch_coarse_distances(a.xq, xb, qn, a.ip ? a.zeros : a.yn + c0, a.matrix, a.nq, (int)nc, a.d, s);
        }
        const float scale = (!direct && a.ip) ? 0.5f : 1.f;
        const dim3 grid((unsigned)((a.nq * P.S + 3) / 4));
        if (P.kpl == 1) hipLaunchKernelGGL(knn_select_kernel<1>, grid, dim3(256), 0, s, a.matrix, nc, a.nq, nc, c0, P.slice_len, P.S, scale, k, a.part, stride);
        else if (P.kpl == 4) hipLaunchKernelGGL(knn_select_kernel<4>, grid, dim3(256), 0, s, a.matrix, nc, a.nq, nc, c0, P.slice_len, P.S, scale, k, a.part, stride);
        else hipLaunchKernelGGL(knn_select_kernel<16>, grid, dim3(256), 0, s, a.matrix, nc, a.nq, nc, c0, P.slice_len, P.S, scale, k, a.part, stride);
        const bool first = c0 == 0, last = c0 + P.chunk >= a.ntotal;
        launch_join_rows(P.kpl, first ? a.part + k : a.part, a.nq, first ? P.S : P.S + 1, stride, k, neg, a.D, a.I, last ? nullptr : a.part, stride, s);
    }
    return true;
}

}  // namespace vlq
