// Product-quantizer training on the device: the assignment of one Lloyd iteration of ALL M sub-quantizers in one launch
// (ProductQuantizer::train, ProductQuantizer.cpp:236-308: M Clustering::train runs on column slices).  pq_train_plan.h has the
// split of the work and the LDS layout.
//   pq_assign_kernel   labels[i][m] = m ksub + argmin_c dis(x_i slice m, cb[m][c]), dis[m][i] = that distance, where
//                      dis = (|x_m|^2 + |c|^2) - 2 ip: ip the k-ordered f32 MFMA chain (= the fmaf chain over k = 0 .. dsub-1 from
//                      0, mfma_tile.cuh), the norms in fvec_norm_L2sqr's order, add, multiply and subtract each rounded -- the
//                      flat search at k = 1 under its GEMM dispatch (scan_knn.hip:112-113), bit for bit.  The winner is the
//                      smallest (dis, column); only a distance below FLT_MAX is admitted (the heap's start).
// and the small kernels of the trainer around it: the initial rows of every slice, the loop route's slice copy and relabel, and
// the residuals of IndexIVFPQ::train_residual_o.
#include "pq_train_plan.h"
#include "mfma_tile.cuh"
#include "sse_order.cuh"
#include "wave_topk.cuh"
#include "kernels.h"

#include <algorithm>

namespace vlq {
namespace {

constexpr float kFltMax = 3.402823466e+38f;
constexpr uint32_t kNoCol = 0xFFFFFFFFu;

// what a lane wrote to its wave's own LDS area is read by the wave's other lanes behind this (LDS accesses of a wave complete
// in order; the fences keep the compiler from moving them)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// TJ 32-column tiles from tile ct0 on against the wave's 32 rows of one slice: TJ independent MFMA chains over the staged k
// pairs, then the epilogue into the lane's running best of its 16 rows.  xa / cb0: the lane's operand rows (parity lane >> 5).
// A padded column's norm is NaN: its distance compares false and is never admitted.
template <int TJ>
__device__ __forceinline__ void pq_col_batch(const float* xa, const float* cb0, const float* cn, int ct0, int kq, int S, int r31,
                                             const float (&qv)[16], float (&best)[16], uint32_t (&bcol)[16]) {
    f32x16 acc[TJ];
#pragma unroll
    for (int tj = 0; tj < TJ; tj++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[tj][r] = 0.f;
    for (int u = 0; u < kq; u++) {
        const float4 av = *reinterpret_cast<const float4*>(xa + 4 * u);
        float4 bv[TJ];
#pragma unroll
        for (int tj = 0; tj < TJ; tj++) bv[tj] = *reinterpret_cast<const float4*>(cb0 + (size_t)((ct0 + tj) * 32 + r31) * S + 4 * u);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float a = e == 0 ? av.x : e == 1 ? av.y : e == 2 ? av.z : av.w;
#pragma unroll
            for (int tj = 0; tj < TJ; tj++) {
                const float b = e == 0 ? bv[tj].x : e == 1 ? bv[tj].y : e == 2 ? bv[tj].z : bv[tj].w;
                acc[tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[tj], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int tj = 0; tj < TJ; tj++) {
        const uint32_t col = (uint32_t)((ct0 + tj) * 32 + r31);
        const float yn = cn[col];
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            // (x_norm + y_norm) - 2 * ip, utils.cpp:884.  Columns arrive in increasing order: the strict test keeps the lower one
            const float dis = __fsub_rn(__fadd_rn(qv[reg], yn), __fmul_rn(2.f, acc[tj][reg]));
            const bool take = dis < best[reg];
            best[reg] = take ? dis : best[reg];
            bcol[reg] = take ? col : bcol[reg];
        }
    }
}

// grid (row-tile walkers, slice groups), 256 threads.  A workgroup stages its group's codebooks once and walks row tiles
// blockIdx.x, blockIdx.x + gridDim.x, ...; wave w owns rows 32 w .. 32 w + 31 of a tile and its own staging area.
template <bool VEC>
__global__ __launch_bounds__(256) void pq_assign_kernel(PqAssignArgs a, int dsub, int ksub, int cols, int kq, int S, int G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    float* cbs = reinterpret_cast<float*>(smraw);                // [G][2 parity][cols][S]
    float* cns = cbs + (size_t)G * 2 * cols * S;                 // [G][cols]
    float* xs_all = cns + (size_t)G * cols;                      // [4 waves][G][2 parity][32][S]
    float* qns_all = xs_all + (size_t)4 * G * 2 * 32 * S;        // [4 waves][G][32]

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int h = lane >> 5, r31 = lane & 31;
    const int m0 = (int)blockIdx.y * G;
    const int gcount = min(G, a.M - m0);
    const int W = gcount * dsub;                                 // floats of a row this workgroup owns: columns m0 dsub ..
    const int64_t n = a.n;

    // the codebooks: zeros everywhere (the k pad, the column pad), then the group's rows; the rows' staging areas start as zeros
    // too (their k pad is never written again)
    for (int e = t; e < G * 2 * cols * S; e += 256) cbs[e] = 0.f;
    for (int e = t; e < 4 * G * 2 * 32 * S; e += 256) xs_all[e] = 0.f;
    for (int e = t; e < G * cols; e += 256) {
        const int g = e / cols, col = e - g * cols;
        cns[e] = (g < gcount && col < ksub) ? a.cnorm[(size_t)(m0 + g) * ksub + col] : __builtin_nanf("");
    }
    __syncthreads();
    {
        const float* src = a.cb + (size_t)m0 * ksub * dsub;
        const int per = ksub * dsub;
        for (int e = t; e < gcount * per; e += 256) {
            const int g = e / per, r = e - g * per;
            const int col = r / dsub, k = r - col * dsub;
            cbs[((size_t)(g * 2 + (k & 1)) * cols + col) * S + (k >> 1)] = src[e];
        }
    }
    __syncthreads();

    float* xs = xs_all + (size_t)wave * G * 2 * 32 * S;
    float* qns = qns_all + wave * G * 32;

    // a lane's place in the staging of a row: unit cu0 (VEC: 4 floats) of row r_off of a pass; its LDS offset without the row
    const int unit = VEC ? 4 : 1;
    const int U = W / unit;
    const int lpr = min(U, 64), rpp = 64 / lpr;
    const int r_off = lane / lpr, cu0 = lane - r_off * lpr;
    const bool stager = lane < rpp * lpr;
    auto lds_off = [&](int c) {                                  // float c of the row part -> [g][parity][0][k >> 1]
        const int g = c / dsub, k = c - g * dsub;
        return ((g * 2 + (k & 1)) * 32) * S + (k >> 1);
    };
    const int loff0 = lds_off(cu0 * unit);

    const int nct = cols / 32;
    const int64_t ntiles = (n + kPqtRows - 1) / kPqtRows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i0 = tile * kPqtRows + wave * 32;
        wave_sync();                                             // the tile before has been read
        if (stager) {
            for (int r = r_off; r < 32; r += rpp) {
                const int64_t row = i0 + r;
                const float* xr = a.x + (size_t)(row < n ? row : 0) * a.d + (size_t)m0 * dsub;
                for (int cu = cu0; cu < U; cu += lpr) {
                    const int lo = (cu == cu0 ? loff0 : lds_off(cu * unit)) + r * S;
                    if constexpr (VEC) {
                        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (row < n) v = *reinterpret_cast<const float4*>(xr + 4 * cu);
                        *reinterpret_cast<float2*>(xs + lo) = make_float2(v.x, v.z);
                        *reinterpret_cast<float2*>(xs + lo + 32 * S) = make_float2(v.y, v.w);
                    } else {
                        xs[lo] = row < n ? xr[cu] : 0.f;
                    }
                }
            }
        }
        wave_sync();
        // |x_m|^2 of (row r31, slice g) in fvec_norm_L2sqr's order, from the staged rows
        for (int g = h; g < gcount; g += 2) {
            const float* xg = xs + (size_t)(g * 2) * 32 * S + r31 * S;
            qns[g * 32 + r31] = norm_sse_order([&](int k) { return xg[(k & 1) * 32 * S + (k >> 1)]; }, dsub);
        }
        wave_sync();

        for (int g = 0; g < gcount; g++) {
            float qv[16], best[16];
            uint32_t bcol[16];
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                qv[reg] = qns[g * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h];
                best[reg] = kFltMax;
                bcol[reg] = kNoCol;
            }
            const float* xa = xs + (size_t)((g * 2 + h) * 32 + r31) * S;
            const float* cb0 = cbs + (size_t)(g * 2 + h) * cols * S;
            const float* cn = cns + g * cols;
            int ct0 = 0;
            for (; ct0 + kPqtColBatch <= nct; ct0 += kPqtColBatch) pq_col_batch<kPqtColBatch>(xa, cb0, cn, ct0, kq, S, r31, qv, best, bcol);
            const int rest = nct - ct0;                          // (wave-uniform)
            if (rest == 3) pq_col_batch<3>(xa, cb0, cn, ct0, kq, S, r31, qv, best, bcol);
            else if (rest == 2) pq_col_batch<2>(xa, cb0, cn, ct0, kq, S, r31, qv, best, bcol);
            else if (rest == 1) pq_col_batch<1>(xa, cb0, cn, ct0, kq, S, r31, qv, best, bcol);

            // a row's winner: the minimum over the 32 lanes of a half of the ordered keys (distance, column).  The key's image of
            // a float orders negative values below positive ones; + 0.f makes -0 the same value as +0.  Lane r31 == reg writes.
            u64 mine = 0;
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                u64 key = make_key(__fadd_rn(best[reg], 0.f), bcol[reg]);
#pragma unroll
                for (int stride = 1; stride < 32; stride <<= 1) {
                    const u64 o = shfl_xor_u64(key, stride);
                    key = o < key ? o : key;
                }
                if (r31 == reg) mine = key;
            }
            if (r31 < 16) {
                const int64_t row = i0 + (r31 & 3) + 8 * (r31 >> 2) + 4 * h;
                if (row < n) {
                    const uint32_t col = (uint32_t)mine;
                    const int m = m0 + g;
                    a.labels[(size_t)row * a.M + m] = col == kNoCol ? (int64_t)-1 : (int64_t)m * ksub + col;
                    a.dis[(size_t)m * n + row] = col == kNoCol ? kFltMax : ordered_to_f32((uint32_t)(mine >> 32));
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void pq_init_rows_kernel(const float* __restrict__ x, const int* __restrict__ perm, int d, int M, int ksub,
                                                           float* __restrict__ cb) {
    const int dsub = d / M;
    const int64_t total = (int64_t)M * ksub * dsub;
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= total) return;
    const int j = (int)(f % dsub);
    const int c = (int)((f / dsub) % ksub);
    const int m = (int)(f / ((int64_t)dsub * ksub));
    cb[f] = x[(size_t)perm[c] * d + (size_t)m * dsub + j];
}

__global__ __launch_bounds__(256) void pq_slice_kernel(const float* __restrict__ x, int64_t n, int d, int dsub, int m, float* __restrict__ out) {
    const int64_t total = n * dsub, step = (int64_t)gridDim.x * 256;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < total; f += step) {
        const int64_t i = f / dsub;
        out[f] = x[(size_t)i * d + (size_t)m * dsub + (f - i * dsub)];
    }
}

__global__ __launch_bounds__(256) void pq_relabel_kernel(const int64_t* __restrict__ local, int64_t n, int M, int m, int ksub,
                                                         int64_t* __restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t l = local[i];
    labels[(size_t)i * M + m] = l < 0 ? -1 : l + (int64_t)m * ksub;
}

// a label outside [0, nlist) raises the flag and leaves the row as it is: nothing is indexed by it
__global__ __launch_bounds__(256) void pq_residual_kernel(const float* __restrict__ x, const int64_t* __restrict__ assign,
                                                          const float* __restrict__ cent, int64_t n, int d, int64_t nlist, float* __restrict__ out,
                                                          int* bad) {
    const int64_t total = n * d, step = (int64_t)gridDim.x * 256;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < total; f += step) {
        const int64_t i = f / d;
        const int64_t c = assign[i];
        if (c < 0 || c >= nlist) { *bad = 1; out[f] = x[f]; continue; }
        out[f] = __fsub_rn(x[f], cent[(size_t)c * d + (f - i * d)]);
    }
}

unsigned blocks_for(int64_t total) { return (unsigned)std::min<int64_t>((total + 255) / 256, 1 << 20); }

}  // namespace

void launch_pq_assign(const PqAssignArgs& a, const PqTrainPlan& P, hipStream_t s) {
    if (a.n <= 0) return;
    if (P.vec && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0) {       // (rows that do not start on 16 bytes: the 4-byte loads)
        ensure_dynamic_lds(reinterpret_cast<const void*>(pq_assign_kernel<true>), P.lds);
        hipLaunchKernelGGL(pq_assign_kernel<true>, P.grid, dim3(256), P.lds, s, a, P.dsub, P.ksub, P.cols, P.kq, P.stride, P.group);
    } else {
        ensure_dynamic_lds(reinterpret_cast<const void*>(pq_assign_kernel<false>), P.lds);
        hipLaunchKernelGGL(pq_assign_kernel<false>, P.grid, dim3(256), P.lds, s, a, P.dsub, P.ksub, P.cols, P.kq, P.stride, P.group);
    }
}

void launch_pq_init_rows(const float* x, const int* perm, int d, int M, int ksub, float* cb, hipStream_t s) {
    const int64_t total = (int64_t)ksub * d;
    hipLaunchKernelGGL(pq_init_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, perm, d, M, ksub, cb);
}

void launch_pq_slice(const float* x, int64_t n, int d, int dsub, int m, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pq_slice_kernel, dim3(blocks_for(n * dsub)), dim3(256), 0, s, x, n, d, dsub, m, out);
}

void launch_pq_relabel(const int64_t* local, int64_t n, int M, int m, int ksub, int64_t* labels, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pq_relabel_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, local, n, M, m, ksub, labels);
}

void launch_pq_residuals(const float* x, const int64_t* assign, const float* centroids, int64_t n, int d, int64_t nlist, float* out, int* bad,
                         hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pq_residual_kernel, dim3(blocks_for(n * d)), dim3(256), 0, s, x, assign, centroids, n, d, nlist, out, bad);
}

}  // namespace vlq
