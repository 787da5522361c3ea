// Flat exact k-NN over float16 rows (vlq_flat_create_ex with storage = 1; GpuIndexFlatConfig::useFloat16): scan_knn.hip's
// search over stored vectors kept as half(x), round to nearest even.  The query stays fp32 and every operation is the fp32
// scan's, in its order; half -> float is exact, so an f16 index over x returns the bits of the fp32 index over float(half(x)).
// Dispatch, routes, row tiles, slices and pages are plan_knn's, with kFlatStoreF16 (knn_plan.h).
//   knn_gemm16_kernel    knn_gemm_kernel with a half B operand.  A thread fetches eight halves of a stored row per unit (one
//                        dwordx4 when d % 8 == 0: half the global-load instructions and half the prefetch registers of the fp32
//                        fragment), and the commit widens them into the same de-interleaved fp32 [2 parity][COLS][S] tile
//                        (mfma_tile.cuh: fetch16 / commit16).  From there on -- MfmaTile::multiply, the accumulators, the epilogue,
//                        the tile-minima admission, the WaveSelect merge -- the code is the fp32 kernel's, and so are the bits.
//                        The A operand (queries) stays fp32.  The fetch of the next step still flies during the MFMA chain.
//   knn_direct16_kernel  knn_direct_kernel's mapping: QT queries as fp32 in LDS, a wave owns 64 rows, a lane one of them.
//                        d % 8 == 0: the 64 x 128 B tile of 64 components a row (flat16_dist.cuh: eight neighbouring lanes fetch
//                        one row's piece, one dwordx4 each) is turned through the wave's LDS area; the lane reads eight halves
//                        with one ds_read_b128, converts them ONCE and feeds the four chains of all QT queries from the converted
//                        registers -- the conversion is paid once per QT pairs, not once per pair as in the IVFFlat scan.  The
//                        next piece's tile is in flight while one is consumed.  d % 8 != 0 (d % 4 == 0): the lane walks its row
//                        by 8-byte loads; correct, not engineered.
//   matrix route, GEMM   (k > 256) a chunk's rows are widened into a bounded fp32 workspace (launch_flat16_decode) and
//                        launch_coarse_distances runs over it unchanged.  No fp32 copy of the index ever stands on the device.
//   knn_select16_kernel, knn_pad16_kernel and the host loop restate scan_knn.hip's knn_select_kernel, knn_pad_kernel and
//                        launch_knn, and knn_gemm16_kernel restates knn_gemm_kernel outside its B operand; that file was to stay
//                        as it is.  Only the tests keep the copies equal: AN EDIT TO THE OPERATION ORDER, THE ADMISSION OR THE KEY
//                        RULES IN ONE MUST BE MIRRORED IN THE OTHER.
//   row_norms16_kernel   |y|^2 of the widened row in fvec_norm_L2sqr's order (launch_row_norms over halves).
#include "kernels.h"
#include "knn_plan.h"
#include "flat16_dist.cuh"
#include "join_rows.cuh"
#include "mfma_tile.cuh"
#include "sse_order.cuh"
#include "wave_topk.cuh"

#include <algorithm>

namespace vlq {

namespace {

constexpr float kFltMax = 3.402823466e+38f;

template <int KPL>
struct KeyRow { u64 best[KPL]; };

template <int WR, int TI, int TJ, int KPL>
__global__ __launch_bounds__(256) void knn_gemm16_kernel(KnnArgs a, int64_t slice_len, int S) {
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
    const _Float16* xh = reinterpret_cast<const _Float16*>(a.xb);       // the stored rows: d halves each

    for (int e = t; e < ROWS * 64 * KPL; e += 256) best[e] = kMaxKey;
    for (int r = t; r < ROWS; r += 256) {
        const bool live = i0 + r < a.nq;
        thrs[r] = live ? kFltMax : -__builtin_inff();                   // a row behind nq admits nothing
        qns[r] = (live && !a.ip) ? a.qn[i0 + r] : 0.f;
    }
    __syncthreads();

    // The walk is knn_gemm_kernel's: the rows of the step after the current one are fetched into registers before the current
    // one is multiplied, and committed (the stored rows widened there) behind it.
    const bool vec_ok = d % 4 == 0;
    const int vec16 = d % 8 == 0 ? 8 : d % 4 == 0 ? 4 : 2;
    typename Tile::template Frag<ROWS> fa;
    typename Tile::template Frag16<COLS> fb;
    if (lo < hi) {
        Tile::template fetch<ROWS>(a.xq, i0, a.nq, d, 0, vec_ok, fa, t);
        Tile::template fetch16<COLS>(xh, lo, hi, d, 0, vec16, fb, t);
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
            Tile::template commit16<COLS>(fb, Tile::lds_b(sm), t);
            __syncthreads();
            const bool more_k = k0 + kKnnKC < d;
            const int64_t jn = more_k ? j0 : j0 + COLS;
            if (jn < hi) {
                const int kn = more_k ? k0 + kKnnKC : 0;
                Tile::template fetch<ROWS>(a.xq, i0, a.nq, d, kn, vec_ok, fa, t);
                Tile::template fetch16<COLS>(xh, jn, hi, d, kn, vec16, fb, t);
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

// eight (four) converted components of the lane's row against the QT queries in LDS: the four chains of every query
template <int QT, bool IP>
__device__ __forceinline__ void direct16_feed8(float (&s)[QT][4], const float* sq, int d, int c, const float (&y)[8]) {
#pragma unroll
    for (int q = 0; q < QT; q++) {
        const f16_v4f x0 = *reinterpret_cast<const f16_v4f*>(sq + q * d + c);        // (one address: a broadcast)
        const f16_v4f x1 = *reinterpret_cast<const f16_v4f*>(sq + q * d + c + 4);
        flat16_acc4<IP>(s[q][0], s[q][1], s[q][2], s[q][3], x0, y[0], y[1], y[2], y[3]);
        flat16_acc4<IP>(s[q][0], s[q][1], s[q][2], s[q][3], x1, y[4], y[5], y[6], y[7]);
    }
}

// out[q][j] = fvec_L2sqr(x_q, float(y_j)) resp. -fvec_inner_product(x_q, float(y_j)) for the QT queries from blockIdx.y * QT on
// and the rows j of the chunk at xb (ncols rows of d halves, d % 4 == 0); a wave owns 64 rows, every lane one of them.
// TILE: d % 8 == 0.
template <int QT, bool IP, bool TILE>
__global__ __launch_bounds__(256) void knn_direct16_kernel(const _Float16* __restrict__ xb, const float* __restrict__ xq, float* __restrict__ out,
                                                           int64_t ld, uint32_t ncols, int nq, int d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    float* sq = reinterpret_cast<float*>(smraw);                                                // [QT][d]
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int q0 = blockIdx.y * QT;
    const int nqt = min(QT, nq - q0);
    for (int e = t; e < QT * d; e += 256) sq[e] = e < nqt * d ? xq[(size_t)q0 * d + e] : 0.f;
    __syncthreads();
    const uint32_t j0 = (blockIdx.x * 4u + (uint32_t)wave) * 64u;
    if (j0 >= ncols) return;
    const uint32_t j = j0 + (uint32_t)lane;
    float s[QT][4];
#pragma unroll
    for (int q = 0; q < QT; q++) s[q][0] = s[q][1] = s[q][2] = s[q][3] = 0.f;
    if constexpr (TILE) {
        float* tile = reinterpret_cast<float*>(smraw + ((size_t)QT * d * 4 + 15) / 16 * 16) + wave * 64 * kFlatTileStride;     // [4][64][kFlatTileStride]
        Flat16Tile cur = flat16_tile_fetch(xb, j0, 0, ncols, d, lane);
        for (int c0 = 0; c0 < d; c0 += kFlat16Chunk) {
            const bool last = c0 + kFlat16Chunk >= d;
            Flat16Tile nxt = cur;
            if (!last) nxt = flat16_tile_fetch(xb, j0, c0 + kFlat16Chunk, ncols, d, lane);
#pragma unroll
            for (int i = 0; i < 8; i++)
                *reinterpret_cast<f16_v4u*>(tile + (i * 8 + (lane >> 3)) * kFlatTileStride + (lane & 7) * 4) = cur.r[i];
            __builtin_amdgcn_wave_barrier();   // (the wave's own area: its LDS accesses complete in order)
            const float* row = tile + lane * kFlatTileStride;
            const int npiece = min(kFlat16Chunk, d - c0) >> 3;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                if (c < npiece) {
                    const f16_h8 h = *reinterpret_cast<const f16_h8*>(row + 4 * c);
                    const float y[8] = {(float)h[0], (float)h[1], (float)h[2], (float)h[3], (float)h[4], (float)h[5], (float)h[6], (float)h[7]};
                    direct16_feed8<QT, IP>(s, sq, d, c0 + 8 * c, y);
                }
            }
            __builtin_amdgcn_wave_barrier();
            cur = nxt;
        }
    } else {
        if (j < ncols) {
            const _Float16* yr = xb + (size_t)j * d;
            for (int i = 0; i < d; i += 4) {
                const f16_h4 h = *reinterpret_cast<const f16_h4*>(yr + i);
                const float y0 = (float)h[0], y1 = (float)h[1], y2 = (float)h[2], y3 = (float)h[3];
#pragma unroll
                for (int q = 0; q < QT; q++)
                    flat16_acc4<IP>(s[q][0], s[q][1], s[q][2], s[q][3], *reinterpret_cast<const f16_v4f*>(sq + q * d + i), y0, y1, y2, y3);
            }
        }
    }
    if (j >= ncols) return;
#pragma unroll
    for (int q = 0; q < QT; q++) {
        const float v = flat16_finish<IP>(s[q][0], s[q][1], s[q][2], s[q][3]);
        if (q < nqt) out[(size_t)(q0 + q) * ld + j] = IP ? flip_sign(v, 0x80000000u) : v;
    }
}

// the k smallest (scale * mat[q][e], col_base + e) of slice s of the chunk -> slot s + 1 of the query's partial rows
template <int KPL>
__global__ __launch_bounds__(256) void knn_select16_kernel(const float* __restrict__ mat, int64_t ld, int64_t nq, int64_t ncols, int64_t col_base,
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
__global__ __launch_bounds__(256) void knn_pad16_kernel(float* __restrict__ D, int64_t* __restrict__ I, int64_t n, float pad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { D[i] = pad; I[i] = -1; }
}

__global__ __launch_bounds__(256) void row_norms16_kernel(const _Float16* __restrict__ x, int64_t n, int d, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const _Float16* xi = x + i * d;
    out[i] = norm_sse_order([&](int c) { return (float)xi[c]; }, d);
}

template <int WR, int TI, int TJ, int KPL>
void launch_gemm16_i(const KnnArgs& a, const KnnPlan& P, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(knn_gemm16_kernel<WR, TI, TJ, KPL>), P.lds);
    const dim3 grid((unsigned)((a.nq + P.rows - 1) / P.rows), (unsigned)P.S);
    hipLaunchKernelGGL((knn_gemm16_kernel<WR, TI, TJ, KPL>), grid, dim3(256), P.lds, s, a, P.slice_len, P.S);
}

template <int QT, bool IP, bool TILE>
void launch_direct16_t(const KnnArgs& a, const KnnPlan& P, const _Float16* xb, int64_t nc, hipStream_t s) {
    const dim3 grid((unsigned)((nc + 255) / 256), (unsigned)((a.nq + QT - 1) / QT));
    ensure_dynamic_lds(reinterpret_cast<const void*>(knn_direct16_kernel<QT, IP, TILE>), P.lds);
    hipLaunchKernelGGL((knn_direct16_kernel<QT, IP, TILE>), grid, dim3(256), P.lds, s, xb, a.xq, a.matrix, nc, (uint32_t)nc, (int)a.nq, a.d);
}

template <int QT>
void launch_direct16_i(const KnnArgs& a, const KnnPlan& P, const _Float16* xb, int64_t nc, hipStream_t s) {
    const bool tile = P.read == kFlatReadTile128;
    if (a.ip) { if (tile) launch_direct16_t<QT, true, true>(a, P, xb, nc, s); else launch_direct16_t<QT, true, false>(a, P, xb, nc, s); }
    else      { if (tile) launch_direct16_t<QT, false, true>(a, P, xb, nc, s); else launch_direct16_t<QT, false, false>(a, P, xb, nc, s); }
}

}  // namespace

void launch_row_norms16(const void* halves, int64_t n, int d, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(row_norms16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const _Float16*>(halves), n, d, out);
}

bool launch_knn16(const KnnArgs& a, const KnnPlan& P, float* widen, hipStream_t s) {
    if (a.nq <= 0) return true;
    if (!P.ok || a.nq > P.page) return false;
    const int k = a.k;
    if (a.ntotal == 0) {
        const int64_t n = a.nq * k;
        hipLaunchKernelGGL(knn_pad16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.D, a.I, n, a.ip ? -kFltMax : kFltMax);
        return true;
    }
    const uint32_t neg = a.ip ? 0x80000000u : 0u;
    if (P.route == kKnnFused) {
        if (P.kpl == 1 && P.rows == 128) launch_gemm16_i<2, 2, 2, 1>(a, P, s);
        else if (P.kpl == 1 && P.rows == 64) launch_gemm16_i<1, 2, 1, 1>(a, P, s);
        else if (P.kpl == 1 && P.rows == 32) launch_gemm16_i<1, 1, 1, 1>(a, P, s);
        else if (P.kpl == 4 && P.rows == 32) launch_gemm16_i<1, 1, 1, 4>(a, P, s);
        else return false;
        if (P.join) launch_join_rows(P.kpl, a.part, a.nq, P.S, (int64_t)P.S * k, k, neg, a.D, a.I, nullptr, 0, s);
        return true;
    }
    // matrix route: chunk by chunk, the running row in slot 0 of the query's S + 1 partial rows
    const int64_t stride = (int64_t)(P.S + 1) * k;
    const bool direct = P.path == kKnnDirect;
    if (!direct && !widen) return false;
    const _Float16* xh = reinterpret_cast<const _Float16*>(a.xb);
    for (int64_t c0 = 0; c0 < a.ntotal; c0 += P.chunk) {
        const int64_t nc = std::min(P.chunk, a.ntotal - c0);
        const _Float16* xb = xh + (size_t)c0 * a.d;
        if (direct) {
            if (P.rows == 19) launch_direct16_i<19>(a, P, xb, nc, s);
            else if (P.rows == 4) launch_direct16_i<4>(a, P, xb, nc, s);
            else if (P.rows == 1) launch_direct16_i<1>(a, P, xb, nc, s);
            else return false;
        } else {
            // the chunk's rows as fp32 (stream order: the previous chunk's distances are done with the workspace), then
            // knn_L2sqr_blas / knn_inner_product_blas as launch_knn runs them
            launch_flat16_decode(xb, nc * a.d, widen, s);
            const float* qn = a.ip ? a.zeros : coarse_norms_fused_ok(a.d) ? nullptr : a.qn;
            launch_coarse_distances(a.xq, widen, qn, a.ip ? a.zeros : a.yn + c0, a.matrix, a.nq, (int)nc, a.d, s);
        }
        const float scale = (!direct && a.ip) ? 0.5f : 1.f;
        const dim3 grid((unsigned)((a.nq * P.S + 3) / 4));
        if (P.kpl == 1) hipLaunchKernelGGL(knn_select16_kernel<1>, grid, dim3(256), 0, s, a.matrix, nc, a.nq, nc, c0, P.slice_len, P.S, scale, k, a.part, stride);
        else if (P.kpl == 4) hipLaunchKernelGGL(knn_select16_kernel<4>, grid, dim3(256), 0, s, a.matrix, nc, a.nq, nc, c0, P.slice_len, P.S, scale, k, a.part, stride);
        else hipLaunchKernelGGL(knn_select16_kernel<16>, grid, dim3(256), 0, s, a.matrix, nc, a.nq, nc, c0, P.slice_len, P.S, scale, k, a.part, stride);
        const bool first = c0 == 0, last = c0 + P.chunk >= a.ntotal;
        launch_join_rows(P.kpl, first ? a.part + k : a.part, a.nq, first ? P.S : P.S + 1, stride, k, neg, a.D, a.I, last ? nullptr : a.part, stride, s);
    }
    return true;
}

}  // namespace vlq
