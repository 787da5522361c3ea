// Range search of the flat index: faiss::IndexFlat::range_search (IndexFlat.cpp:58-70; range_search_L2sqr /
// range_search_inner_product, utils.cpp:1090-1262) on the device.  Every stored vector with
//   L2            dis < radius        inner product   ip > radius      (strict; a NaN on either side is no hit; no clamp)
// is a hit, and a query's hits come out in ascending position.  Distances are the k-NN scan's bit for bit (scan_knn.hip): the
// dispatch, the expressions and their operation order are the same, only the selection is gone.  Path, row tile and slices
// are plan_knn_range's decision (knn_range_plan.h).
//   range_gemm_kernel    A workgroup owns ROWS queries and walks the 128-column tiles of its slice with MfmaTile and the
//                        fetch-ahead of knn_gemm_kernel.  The epilogue tests (x_norm + y_norm) - 2 ip resp. ip against the radius
//                        in registers; one ballot per accumulator register is the 32-column hit word of two rows, and the words
//                        of a tile go to LDS as [ROWS][4] masks.
//   range_direct_kernel  nq < 20 && d % 4 == 0: knn_direct_kernel's walk (the call's queries in LDS, a wave turns 64 rows through
//                        its LDS tile, a lane scores its row for all QT queries), the workgroup walking its slice in 256-row trips.
// The output is variable-length and ordered, so both kernels run twice, as the IVFFlat range scan does (scan_range_flat.hip):
//   count (FILL = false)  popcounts; counts[q][slice] at the end.  One exclusive scan over the flattened counts gives base.
//   fill  (FILL = true)   the distances again; a hit goes to slot base[q][slice] + the row's running count + the popcount of the
//                         hit bits in front of its column.  No atomics, no sort: the order comes out of the addressing.
// Both passes run the same barriers through the same tiles; rows, clamps and validity are the same expressions in both.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "kernels.h"
#include "knn_range_plan.h"
#include "flat_dist.cuh"
#include "mfma_tile.cuh"

namespace vlq {

namespace {

template <int WR, int TI, int TJ, bool FILL>
__global__ __launch_bounds__(256) void range_gemm_kernel(KnnRangeArgs a, int64_t slice_len, int S) {
    typedef MfmaTile<kKnnKC, WR, TI, TJ> Tile;
    constexpr int ROWS = Tile::ROWS, COLS = Tile::COLS, WC = Tile::WC, NW = COLS / 32;
    static_assert(COLS == kKnnColTile, "the plan's column tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    float* sm = reinterpret_cast<float*>(smraw);                                // the staged tiles
    uint32_t* masks = reinterpret_cast<uint32_t*>(sm + Tile::kLdsFloats);       // [ROWS][NW] hit words of the current tile
    uint32_t* runs = masks + ROWS * NW;                                         // [ROWS] hits of the row in the tiles before (fill)
    float* qns = reinterpret_cast<float*>(runs + ROWS);                         // [ROWS] |q|^2

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave / WC, wc = wave % WC;
    const int64_t i0 = (int64_t)blockIdx.x * ROWS;
    const int slice = blockIdx.y;
    const int64_t lo = min((int64_t)slice * slice_len, a.ntotal), hi = min(lo + slice_len, a.ntotal);
    const int d = a.d;
    const int nlive = (int)min((int64_t)ROWS, a.nq - i0);                       // a row behind nq is never a hit
    const float radius = a.radius;

    for (int r = t; r < ROWS; r += 256) qns[r] = (r < nlive && !a.ip) ? a.qn[i0 + r] : 0.f;
    uint32_t myrun = 0;                 // thread t < ROWS: the hits of row t in the tiles walked so far
    __syncthreads();

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
            __syncthreads();
        }

        // the hit words of the tile: lanes 0 .. 31 hold the 32 columns of row (reg & 3) + 8 (reg >> 2), lanes 32 .. 63 those of
        // the row 4 below, so one ballot is the words of both.  (masks and runs were last read before the barriers of the k loop)
        const int h = lane >> 5, cidx = lane & 31;
        if (FILL && t < ROWS) runs[t] = myrun;
#pragma unroll
        for (int tj = 0; tj < TJ; tj++) {
            const int64_t col = j0 + (wc * TJ + tj) * 32 + cidx;
            const bool live = col < hi;                 // a column behind the slice's end is never a hit
            const float ynv = (live && !a.ip) ? a.yn[col] : 0.f;
#pragma unroll
            for (int ti = 0; ti < TI; ti++) {
#pragma unroll
                for (int reg = 0; reg < 16; reg++) {
                    const int rowl = (wr * TI + ti) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    const float ip = acc[ti][tj][reg];
                    // (x_norm + y_norm) - 2 * ip, utils.cpp:1148; inner product: ip
                    const float dis = a.ip ? ip : __fsub_rn(__fadd_rn(qns[rowl], ynv), __fmul_rn(2.f, ip));
                    const bool hit = live && rowl < nlive && (a.ip ? dis > radius : dis < radius);
                    const unsigned long long bal = __ballot(hit);
                    if (cidx == 0) masks[rowl * NW + wc * TJ + tj] = h ? (uint32_t)(bal >> 32) : (uint32_t)bal;
                }
            }
        }
        __syncthreads();

        if constexpr (FILL) {
#pragma unroll
            for (int tj = 0; tj < TJ; tj++) {
                const int w = wc * TJ + tj;
                const int64_t col = j0 + w * 32 + cidx;
                const bool live = col < hi;
                const float ynv = (live && !a.ip) ? a.yn[col] : 0.f;
#pragma unroll
                for (int ti = 0; ti < TI; ti++) {
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) {
                        const int rowl = (wr * TI + ti) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                        const float ip = acc[ti][tj][reg];
                        const float dis = a.ip ? ip : __fsub_rn(__fadd_rn(qns[rowl], ynv), __fmul_rn(2.f, ip));
                        const bool hit = live && rowl < nlive && (a.ip ? dis > radius : dis < radius);
                        const unsigned long long bal = __ballot(hit);
                        if (bal == 0) continue;         // (wave-uniform) almost every register of almost every tile
                        if (hit) {
                            const uint32_t mine = h ? (uint32_t)(bal >> 32) : (uint32_t)bal;
                            uint32_t r = runs[rowl] + (uint32_t)__popc(mine & ((1u << cidx) - 1u));
                            for (int ww = 0; ww < w; ww++) r += (uint32_t)__popc(masks[rowl * NW + ww]);
                            const int64_t slot = a.base[(i0 + rowl) * S + slice] + (int64_t)r;
                            if (slot < a.total) {       // (always: the count pass saw the same hits)
                                a.D[slot] = dis;
                                a.I[slot] = col;
                            }
                        }
                    }
                }
            }
        }
        if (t < ROWS) {
            uint32_t c = 0;
#pragma unroll
            for (int ww = 0; ww < NW; ww++) c += (uint32_t)__popc(masks[t * NW + ww]);
            myrun += c;
        }
    }

    if constexpr (!FILL) {
        if (t < nlive) a.counts[(i0 + t) * S + slice] = myrun;
    }
}

// knn_direct_kernel's scores of rows j0 .. j0 + 63 (lane l: row min(j0 + l, len - 1)) against the QT queries in sq [QT][d]:
// fvec_L2sqr / fvec_inner_product in the reference's order.  `cur` holds the rows' first tile on entry and that of rows
// j_next .. on return (flat_dist.cuh: in flight while the last piece is consumed).
template <int QT, bool IP>
__device__ __forceinline__ void range_direct_scores(const float* __restrict__ xb, uint32_t j0, uint32_t j_next, uint32_t len, int d, int lane,
                                                    float* tile, const float* sq, FlatTile& cur, float (&v)[QT]) {
    float s[QT][4];
#pragma unroll
    for (int q = 0; q < QT; q++) s[q][0] = s[q][1] = s[q][2] = s[q][3] = 0.f;
    for (int c0 = 0; c0 < d; c0 += kFlatChunk) {
        const bool last = c0 + kFlatChunk >= d;
        const FlatTile nxt = flat_tile_fetch(xb, last ? j_next : j0, last ? 0 : c0 + kFlatChunk, len, d, lane);
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
#pragma unroll
    for (int q = 0; q < QT; q++) {
        float s0 = s[q][0], s1 = s[q][1], s2 = s[q][2], s3 = s[q][3];
        if constexpr (IP) {     // the tail term of fvec_inner_product is added whatever d is (utils.cpp:527-530)
            s0 = __fadd_rn(s0, 0.f); s1 = __fadd_rn(s1, 0.f); s2 = __fadd_rn(s2, 0.f); s3 = __fadd_rn(s3, 0.f);
        }
        v[q] = __fadd_rn(__fadd_rn(s0, s1), __fadd_rn(s2, s3));
    }
}

// grid (slice) x (group of QT queries); d % 4 == 0
template <int QT, bool IP, bool FILL>
__global__ __launch_bounds__(256) void range_direct_kernel(KnnRangeArgs a, int64_t slice_len, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    const int d = a.d;
    float* sq = reinterpret_cast<float*>(smraw);                                                // [QT][d]
    float* tiles = reinterpret_cast<float*>(smraw + ((size_t)QT * d * 4 + 15) / 16 * 16);       // [4][64][kFlatTileStride]
    uint32_t* xch = reinterpret_cast<uint32_t*>(tiles + 4 * 64 * kFlatTileStride);              // [2][4][QT] hit counts of a trip
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int slice = blockIdx.x;
    const int q0 = blockIdx.y * QT;
    const int nqt = (int)min((int64_t)QT, a.nq - q0);
    const int64_t lo = min((int64_t)slice * slice_len, a.ntotal), hi = min(lo + slice_len, a.ntotal);
    const float radius = a.radius;
    for (int e = t; e < QT * d; e += 256) sq[e] = e < nqt * d ? a.xq[(size_t)q0 * d + e] : 0.f;
    __syncthreads();

    // count: the hits of this wave's groups.  fill: the slot of the workgroup's next hit, the same value in every wave
    unsigned long long run[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) run[q] = (FILL && q < nqt) ? (unsigned long long)a.base[(int64_t)(q0 + q) * S + slice] : 0ull;
    int set = 0;
    float* tile = tiles + wave * 64 * kFlatTileStride;
    const uint32_t len = (uint32_t)hi;                  // (ntotal < 2^32) rows are clamped to the slice's end
    FlatTile cur = {};
    if (lo + wave * 64 < hi) cur = flat_tile_fetch(a.xb, (uint32_t)(lo + wave * 64), 0, len, d, lane);
    for (int64_t t0 = lo; t0 < hi; t0 += kKnnRangeTrip) {      // (workgroup-uniform trips)
        const int64_t j0 = t0 + wave * 64, j = j0 + lane;
        const bool active = j0 < hi;                    // (wave-uniform; once false it stays false)
        float v[QT];
#pragma unroll
        for (int q = 0; q < QT; q++) v[q] = 0.f;
        if (active) {
            const uint32_t j_next = (uint32_t)min(j0 + kKnnRangeTrip, hi - 1);
            range_direct_scores<QT, IP>(a.xb, (uint32_t)j0, j_next, len, d, lane, tile, sq, cur, v);
        }
        unsigned long long mask[QT];
#pragma unroll
        for (int q = 0; q < QT; q++) {
            const bool hit = active && j < hi && q < nqt && (IP ? v[q] > radius : v[q] < radius);
            mask[q] = __ballot(hit);
        }
        if constexpr (!FILL) {
#pragma unroll
            for (int q = 0; q < QT; q++) run[q] += (unsigned long long)__popcll(mask[q]);
        } else {
            uint32_t* mine = xch + (set * 4 + wave) * QT;
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < QT; q++) mine[q] = (uint32_t)__popcll(mask[q]);
            }
            __syncthreads();
            const uint32_t* xs = xch + set * 4 * QT;
            set ^= 1;
            const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
            for (int q = 0; q < QT; q++) {
                const uint32_t c0 = xs[q], c1 = xs[QT + q], c2 = xs[2 * QT + q], c3 = xs[3 * QT + q];
                const unsigned long long slot = run[q] + (wave > 0 ? c0 : 0u) + (wave > 1 ? c1 : 0u) + (wave > 2 ? c2 : 0u) +
                                                (unsigned long long)__popcll(mask[q] & below);
                run[q] += (unsigned long long)c0 + c1 + c2 + c3;
                if (((mask[q] >> lane) & 1ull) && slot < (unsigned long long)a.total) {     // (slot < total always)
                    a.D[slot] = v[q];
                    a.I[slot] = j;
                }
            }
        }
    }

    if constexpr (!FILL) {
        __syncthreads();                                // (the row tiles are read no more: their area takes the waves' counts)
        unsigned long long* w = reinterpret_cast<unsigned long long*>(tiles);       // [4][QT]
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < QT; q++) w[wave * QT + q] = run[q];
        }
        __syncthreads();
        if (t < nqt) a.counts[(int64_t)(q0 + t) * S + slice] = (uint32_t)(w[t] + w[QT + t] + w[2 * QT + t] + w[3 * QT + t]);
    }
}

__global__ __launch_bounds__(256) void range_lims_kernel(const int64_t* __restrict__ base, int64_t n, int S, int64_t* __restrict__ lims) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q <= n) lims[q] = base[q * S];
}

struct CountToSlot {
    __host__ __device__ int64_t operator()(uint32_t c) const { return (int64_t)c; }
};

template <int WR, int TI, int TJ>
void launch_gemm_i(const KnnRangeArgs& a, const KnnRangePlan& P, bool fill, hipStream_t s) {
    const dim3 grid((unsigned)((a.nq + P.rows - 1) / P.rows), (unsigned)P.S);
    if (fill) {
        ensure_dynamic_lds(reinterpret_cast<const void*>(range_gemm_kernel<WR, TI, TJ, true>), P.lds);
        hipLaunchKernelGGL((range_gemm_kernel<WR, TI, TJ, true>), grid, dim3(256), P.lds, s, a, P.slice_len, P.S);
    } else {
        ensure_dynamic_lds(reinterpret_cast<const void*>(range_gemm_kernel<WR, TI, TJ, false>), P.lds);
        hipLaunchKernelGGL((range_gemm_kernel<WR, TI, TJ, false>), grid, dim3(256), P.lds, s, a, P.slice_len, P.S);
    }
}

template <int QT, bool IP>
void launch_direct_ii(const KnnRangeArgs& a, const KnnRangePlan& P, bool fill, hipStream_t s) {
    const dim3 grid((unsigned)P.S, (unsigned)((a.nq + QT - 1) / QT));
    if (fill) {
        ensure_dynamic_lds(reinterpret_cast<const void*>(range_direct_kernel<QT, IP, true>), P.lds);
        hipLaunchKernelGGL((range_direct_kernel<QT, IP, true>), grid, dim3(256), P.lds, s, a, P.slice_len, P.S);
    } else {
        ensure_dynamic_lds(reinterpret_cast<const void*>(range_direct_kernel<QT, IP, false>), P.lds);
        hipLaunchKernelGGL((range_direct_kernel<QT, IP, false>), grid, dim3(256), P.lds, s, a, P.slice_len, P.S);
    }
}

template <int QT>
void launch_direct_i(const KnnRangeArgs& a, const KnnRangePlan& P, bool fill, hipStream_t s) {
    if (a.ip) launch_direct_ii<QT, true>(a, P, fill, s);
    else launch_direct_ii<QT, false>(a, P, fill, s);
}

}  // namespace

bool launch_knn_range(const KnnRangeArgs& a, const KnnRangePlan& P, bool fill, hipStream_t s) {
    if (a.nq <= 0) return true;
    if (!P.ok || a.nq > P.page || a.ntotal <= 0) return false;
    if (P.path == kKnnGemm) {
        if (P.rows == 128) launch_gemm_i<2, 2, 2>(a, P, fill, s);
        else if (P.rows == 64) launch_gemm_i<1, 2, 1>(a, P, fill, s);
        else if (P.rows == 32) launch_gemm_i<1, 1, 1>(a, P, fill, s);
        else return false;
        return true;
    }
    if (a.d % 4 != 0) return false;
    if (P.rows == 19) launch_direct_i<19>(a, P, fill, s);
    else if (P.rows == 4) launch_direct_i<4>(a, P, fill, s);
    else if (P.rows == 1) launch_direct_i<1>(a, P, fill, s);
    else return false;
    return true;
}

hipError_t knn_range_scan(const uint32_t* c, int64_t* base, int64_t n, void* tmp, size_t* tmp_bytes, hipStream_t s) {
    return rocprim::exclusive_scan(tmp, *tmp_bytes, rocprim::make_transform_iterator(c, CountToSlot()), base, (int64_t)0, (size_t)n,
                                   rocprim::plus<int64_t>(), s);
}

void launch_knn_range_lims(const int64_t* base, int64_t n, int S, int64_t* lims, hipStream_t s) {
    hipLaunchKernelGGL(range_lims_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, base, n, S, lims);
}

}  // namespace vlq
