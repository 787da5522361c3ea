// The f32 MFMA inner-product tile shared by the distance kernels (kernels.hip: coarse_dist_kernel; scan_knn.hip:
// knn_gemm_kernel): a 256-thread workgroup computes <a_i, b_j> for ROWS x COLS pairs, every element a chain over
// k = 0, 1, 2, ... in natural order -- bit-identical to a scalar fmaf chain from 0, whatever the tile shape.
//
// Four waves as WR x WC (WC = 4 / WR), each wave TI x TJ v_mfma_f32_32x32x2_f32 accumulators of 32 x 32.  The MFMA consumes k
// in pairs (lane >> 5 selects the parity), so the LDS tiles are stored de-interleaved (even k | odd k): every lane reads
// 4 consecutive k-pairs with one ds_read_b128.  Row stride KC / 2 + 4 floats keeps the b128 reads bank-conflict free.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vlq {

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int KC, int WR, int TI, int TJ>
struct MfmaTile {
    static constexpr int S = KC / 2 + 4;                 // floats between the rows of a staged tile
    static constexpr int WC = 4 / WR;
    static constexpr int ROWS = WR * TI * 32, COLS = WC * TJ * 32;
    static constexpr int kLdsFloats = 2 * (ROWS + COLS) * S;      // [2 parity][ROWS][S] of A, then [2 parity][COLS][S] of B

    // The staging of N rows is split in two, so that a caller can keep the loads of the next step in flight while it multiplies:
    // fetch: rows n0 .. n0 + N - 1 of x [lim][d] (zeros behind lim and behind d), floats k0 .. k0 + KC - 1, into registers;
    // commit: the registers into dst [2 parity][N][S]
    template <int N>
    struct Frag { float4 v[N * (KC / 4) / 256]; };
    template <int N>
    static __device__ __forceinline__ void fetch(const float* __restrict__ x, int64_t n0, int64_t lim, int d, int k0, bool vec_ok,
                                                 Frag<N>& fr, int t) {
        static_assert(N * (KC / 4) % 256 == 0, "whole trips of the 256 threads");
#pragma unroll
        for (int i = 0; i < N * (KC / 4) / 256; i++) {
            const int f = t + i * 256;
            const int row = f / (KC / 4), v = f % (KC / 4);
            const int kk = k0 + 4 * v;
            const int64_t grow = n0 + row;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (grow < lim) {
                const float* p = x + grow * d + kk;
                if (vec_ok && kk + 4 <= d) {
                    val = *reinterpret_cast<const float4*>(p);
                } else {
                    if (kk + 0 < d) val.x = p[0];
                    if (kk + 1 < d) val.y = p[1];
                    if (kk + 2 < d) val.z = p[2];
                    if (kk + 3 < d) val.w = p[3];
                }
            }
            fr.v[i] = val;
        }
    }
    template <int N>
    static __device__ __forceinline__ void commit(const Frag<N>& fr, float* dst, int t) {
#pragma unroll
        for (int i = 0; i < N * (KC / 4) / 256; i++) {
            const int f = t + i * 256;
            const int row = f / (KC / 4), v = f % (KC / 4);
            const float4 val = fr.v[i];
            *reinterpret_cast<float2*>(dst + (0 * N + row) * S + 2 * v) = make_float2(val.x, val.z);
            *reinterpret_cast<float2*>(dst + (1 * N + row) * S + 2 * v) = make_float2(val.y, val.w);
        }
    }

    static __device__ __forceinline__ float* lds_a(float* sm) { return sm; }
    static __device__ __forceinline__ float* lds_b(float* sm) { return sm + 2 * ROWS * S; }

    // acc[ti][tj] += <A rows, B rows> over the KC floats staged in sm (the arithmetic: k in natural order)
    // C/D layout of an accumulator: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    static __device__ __forceinline__ void multiply(const float* sm, f32x16 (&acc)[TI][TJ]) {
        const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
        const int wr = wave / WC, wc = wave % WC;
        const float* sa = sm;
        const float* sb = sm + 2 * ROWS * S;
        const int h = lane >> 5, r = lane & 31;
#pragma unroll
        for (int u = 0; u < KC / 8; u++) {
            float4 a[TI], b[TJ];
#pragma unroll
            for (int ti = 0; ti < TI; ti++)
                a[ti] = *reinterpret_cast<const float4*>(sa + (h * ROWS + (wr * TI + ti) * 32 + r) * S + 4 * u);
#pragma unroll
            for (int tj = 0; tj < TJ; tj++)
                b[tj] = *reinterpret_cast<const float4*>(sb + (h * COLS + (wc * TJ + tj) * 32 + r) * S + 4 * u);
#pragma unroll
            for (int e = 0; e < 4; e++) {
#pragma unroll
                for (int ti = 0; ti < TI; ti++)
#pragma unroll
                    for (int tj = 0; tj < TJ; tj++) {
                        const float av = e == 0 ? a[ti].x : e == 1 ? a[ti].y : e == 2 ? a[ti].z : a[ti].w;
                        const float bv = e == 0 ? b[tj].x : e == 1 ? b[tj].y : e == 2 ? b[tj].z : b[tj].w;
                        acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[ti][tj], 0, 0, 0);
                    }
            }
        }
    }

    // acc[ti][tj] += <A rows, B rows> over the whole k range; sm: kLdsFloats floats.  Ends behind a barrier: sm is free.
    static __device__ __forceinline__ void accumulate(const float* __restrict__ A, int64_t i0, int64_t na, const float* __restrict__ B,
                                                      int64_t j0, int64_t nb, int d, float* sm, f32x16 (&acc)[TI][TJ]) {
        const int t = threadIdx.x;
        const bool vec_ok = (d % 4 == 0);
        for (int k0 = 0; k0 < d; k0 += KC) {
            Frag<ROWS> fa;
            Frag<COLS> fb;
            fetch<ROWS>(A, i0, na, d, k0, vec_ok, fa, t);
            fetch<COLS>(B, j0, nb, d, k0, vec_ok, fb, t);
            commit<ROWS>(fa, lds_a(sm), t);
            commit<COLS>(fb, lds_b(sm), t);
            __syncthreads();
            multiply(sm, acc);
            __syncthreads();
        }
    }
};

}  // namespace vlq
