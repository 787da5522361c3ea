// The kernels of the vector transforms (include/vlq_ivfpq.h, vlq_transform_*; the launch decision: transform_plan.h).
//
// linear_strip_kernel: xt = b + x A^T as a tall-skinny product.  A workgroup of four waves owns a strip of 128 rows of x and
// walks ALL column panels of the matrix for it, so x is read from HBM once and xt written once; the matrix (d_out * d_in
// floats, a few hundred KB at most) is re-read per strip from L2.  The four waves sit 2 x 2 over the 128 x 128 tile, each with
// 2 x 2 accumulators of v_mfma_f32_32x32x2_f32: the strip's rows are the MFMA's A operand and the matrix rows its B operand, so
// in the accumulator layout lane & 31 runs along j and a half-wave stores 128 contiguous bytes of a row of xt.
//   LDS: operands de-interleaved by k parity as in mfma_tile.cuh ([2][rows][stride], one ds_read_b128 = four k-pairs).
//   RESIDENT (d_in <= kMaxResidentD): the whole strip [2][128][kp / 2 + 4] is staged once and every panel reads it; only the
//   matrix moves, 32 floats of k at a step through two buffers: step s + 1 is loaded into registers before the MFMAs of step
//   s are issued and committed to the other buffer behind them, one barrier a step.
//   otherwise the strip is staged step by step beside the matrix (and re-read per panel, from L2 mostly); the accumulators
//   live across the steps of a panel either way, so the chain over k is the same: natural order, starting from the bias.
//   Padding: rows behind n and behind d_out are zeros.  Behind d_in the strip is padded with 0.0f and the MATRIX with -1.0f: the
//   padded products are -0.0f, the one addend that leaves every accumulator as it is (-0.0f included).
// linear_rows_kernel: the same chain on the VALU for a handful of rows: a wave per (row, 64 outputs); a 64 x 64 tile of the
// matrix is read coalesced along i into LDS and shared by the block's four rows, x[r] is broadcast from LDS.
#include "transform_plan.h"

#include "kernels.h"
#include "mfma_tile.cuh"
#include "sse_order.cuh"

namespace vlq {
namespace {

constexpr int kStepFloats = 2 * kPanelCols * kStepStride;     // one staged step of 128 rows
static_assert(kStripRows == 128 && kPanelCols == 128 && kStepK == 32, "the staging below is written for 128 x 128 x 32 and 256 threads");

// floats k .. k + 3 of row `row` of m [lim][d]: zeros behind lim, `pad` behind d
__device__ __forceinline__ float4 load4(const float* __restrict__ m, int64_t row, int64_t lim, int d, int k, bool vec_ok, float pad) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < lim) {
        const float* p = m + row * d + k;
        if (vec_ok && k + 4 <= d) {
            v = *reinterpret_cast<const float4*>(p);
        } else {
            v.x = k + 0 < d ? p[0] : pad;
            v.y = k + 1 < d ? p[1] : pad;
            v.z = k + 2 < d ? p[2] : pad;
            v.w = k + 3 < d ? p[3] : pad;
        }
    }
    return v;
}

// ... of the strip: x[row][k ..] - sub[k ..], the difference rounded (transform_transpose's y_new)
__device__ __forceinline__ float4 load_x(const LinearArgs& a, int64_t row, int k, bool vec_ok) {
    float4 v = load4(a.x, row, a.n, a.d_in, k, vec_ok, 0.f);
    if (a.sub) {
        if (k + 0 < a.d_in) v.x = __fsub_rn(v.x, a.sub[k + 0]);
        if (k + 1 < a.d_in) v.y = __fsub_rn(v.y, a.sub[k + 1]);
        if (k + 2 < a.d_in) v.z = __fsub_rn(v.z, a.sub[k + 2]);
        if (k + 3 < a.d_in) v.w = __fsub_rn(v.w, a.sub[k + 3]);
    }
    return v;
}

// four floats of k = 4 v .. 4 v + 3 into dst [2 parity][128][S]
__device__ __forceinline__ void put4(float* dst, int S, int row, int v, float4 val) {
    *reinterpret_cast<float2*>(dst + (0 * 128 + row) * S + 2 * v) = make_float2(val.x, val.z);
    *reinterpret_cast<float2*>(dst + (1 * 128 + row) * S + 2 * v) = make_float2(val.y, val.w);
}

// acc += <strip rows, matrix rows> over one step of kStepK floats; sa: the strip's step (row stride Sa), sb: the matrix's
__device__ __forceinline__ void multiply_step(const float* sa, int Sa, const float* sb, f32x16 (&acc)[2][2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1, h = lane >> 5, r = lane & 31;
#pragma unroll
    for (int u = 0; u < kStepK / 8; u++) {
        float4 a[2], b[2];
#pragma unroll
        for (int ti = 0; ti < 2; ti++) a[ti] = *reinterpret_cast<const float4*>(sa + (h * kStripRows + (wr * 2 + ti) * 32 + r) * Sa + 4 * u);
#pragma unroll
        for (int tj = 0; tj < 2; tj++) b[tj] = *reinterpret_cast<const float4*>(sb + (h * kPanelCols + (wc * 2 + tj) * 32 + r) * kStepStride + 4 * u);
#pragma unroll
        for (int e = 0; e < 4; e++) {
#pragma unroll
            for (int ti = 0; ti < 2; ti++)
#pragma unroll
                for (int tj = 0; tj < 2; tj++) {
                    const float av = e == 0 ? a[ti].x : e == 1 ? a[ti].y : e == 2 ? a[ti].z : a[ti].w;
                    const float bv = e == 0 ? b[tj].x : e == 1 ? b[tj].y : e == 2 ? b[tj].z : b[tj].w;
                    acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[ti][tj], 0, 0, 0);
                }
        }
    }
}

template <bool RESIDENT>
__global__ __launch_bounds__(256) void linear_strip_kernel(LinearArgs a, bool vec_x, bool vec_a) {
    extern __shared__ float4 strip_smem[];
    float* sm = reinterpret_cast<float*>(strip_smem);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t i0 = (int64_t)blockIdx.x * kStripRows;
    const int kp = (a.d_in + kStepK - 1) / kStepK * kStepK;
    const int nch = kp / kStepK, npanel = (a.d_out + kPanelCols - 1) / kPanelCols;
    const int Sx = RESIDENT ? kp / 2 + 4 : kStepStride;
    float* sx = sm;
    float* sA = sm + (RESIDENT ? 2 * kStripRows * Sx : 2 * kStepFloats);

    float4 fa[4], fx[4];
    auto fetch_a = [&](int p, int c) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int f = t + i * 256;
            fa[i] = load4(a.A, (int64_t)p * kPanelCols + (f >> 3), a.d_out, a.d_in, c * kStepK + 4 * (f & 7), vec_a, -1.f);
        }
    };
    auto fetch_x = [&](int c) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int f = t + i * 256;
            fx[i] = load_x(a, i0 + (f >> 3), c * kStepK + 4 * (f & 7), vec_x);
        }
    };
    auto commit = [&](const float4 (&fr)[4], float* dst) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int f = t + i * 256;
            put4(dst, kStepStride, f >> 3, f & 7, fr[i]);
        }
    };

    fetch_a(0, 0);
    commit(fa, sA);
    if (RESIDENT) {
        const int vpr = kp / 4;                                   // float4 per row of the strip
        for (int f = t; f < kStripRows * vpr; f += 256) {
            const int row = f / vpr, v = f - row * vpr;
            put4(sx, Sx, row, v, load_x(a, i0 + row, 4 * v, vec_x));
        }
    } else {
        fetch_x(0);
        commit(fx, sx);
    }
    __syncthreads();

    f32x16 acc[2][2];
    int s = 0;
    for (int p = 0; p < npanel; p++) {
#pragma unroll
        for (int tj = 0; tj < 2; tj++) {
            const int j = p * kPanelCols + (wc * 2 + tj) * 32 + (lane & 31);
            const float bv = (a.bias && j < a.d_out) ? a.bias[j] : 0.f;          // the chain STARTS from the bias
#pragma unroll
            for (int ti = 0; ti < 2; ti++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[ti][tj][e] = bv;
        }
        for (int c = 0; c < nch; c++, s++) {
            const bool more = c + 1 < nch || p + 1 < npanel;
            const int cn = c + 1 < nch ? c + 1 : 0, pn = c + 1 < nch ? p : p + 1;
            if (more) {                                           // the next step's loads fly during this step's MFMAs
                fetch_a(pn, cn);
                if (!RESIDENT) fetch_x(cn);
            }
            multiply_step(RESIDENT ? sx + (kStepK / 2) * c : sx + (s & 1) * kStepFloats, Sx, sA + (s & 1) * kStepFloats, acc);
            if (more) {
                commit(fa, sA + ((s + 1) & 1) * kStepFloats);
                if (!RESIDENT) commit(fx, sx + ((s + 1) & 1) * kStepFloats);
            }
            __syncthreads();
        }
        // C/D layout of an accumulator: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int ti = 0; ti < 2; ti++)
#pragma unroll
            for (int tj = 0; tj < 2; tj++) {
                const int j = p * kPanelCols + (wc * 2 + tj) * 32 + (lane & 31);
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int64_t row = i0 + (wr * 2 + ti) * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                    if (row < a.n && j < a.d_out) a.xt[row * a.d_out + j] = acc[ti][tj][e];
                }
            }
    }
}

__global__ __launch_bounds__(256) void linear_rows_kernel(LinearArgs a) {
    __shared__ float sA[kRowsCols][kRowsStepK + 1];
    __shared__ float sxr[kRowsPerBlock][kRowsStepK];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j0 = blockIdx.x * kRowsCols, j = j0 + lane;
    const int64_t r = (int64_t)blockIdx.y * kRowsPerBlock + w;
    float acc = (a.bias && j < a.d_out) ? a.bias[j] : 0.f;
    for (int k0 = 0; k0 < a.d_in; k0 += kRowsStepK) {
        const int kn = min(kRowsStepK, a.d_in - k0);
        const bool k_ok = lane < kn;
        for (int jj = w; jj < kRowsCols; jj += kRowsPerBlock)
            sA[jj][lane] = (k_ok && j0 + jj < a.d_out) ? a.A[(int64_t)(j0 + jj) * a.d_in + k0 + lane] : 0.f;
        float xv = 0.f;
        if (k_ok && r < a.n) {
            xv = a.x[r * a.d_in + k0 + lane];
            if (a.sub) xv = __fsub_rn(xv, a.sub[k0 + lane]);
        }
        sxr[w][lane] = xv;
        __syncthreads();
        for (int i = 0; i < kn; i++) acc = fmaf(sA[lane][i], sxr[w][i], acc);
        __syncthreads();
    }
    if (r < a.n && j < a.d_out) a.xt[r * a.d_out + j] = acc;
}

__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ A, float* __restrict__ At, int rows, int cols) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < rows && c0 + tx < cols) tile[i][tx] = A[(int64_t)(r0 + i) * cols + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < cols && r0 + tx < rows) At[(int64_t)(c0 + i) * rows + r0 + tx] = tile[tx][i];
}

__global__ __launch_bounds__(256) void remap_kernel(const float* __restrict__ x, float* __restrict__ xt, int64_t n, int d_src, int d_dst,
                                                    const int* __restrict__ map) {
    const int64_t total = n * d_dst, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < total; f += step) {
        const int64_t r = f / d_dst;
        const int m = map[f - r * d_dst];
        xt[f] = (m < 0 || m >= d_src) ? 0.f : x[r * d_src + m];
    }
}

// fvec_renorm_L2 (utils.cpp:686-701): a wave per row; the norm in the SSE order (every lane runs the same four chains over
// the row, one address per load), then the lanes share the row's components.  The chains are serial in d and 64 times
// redundant: correct and in the stated order, but not timed -- a chain [PCA, L2norm] pays it per batch
__global__ __launch_bounds__(256) void l2norm_kernel(const float* __restrict__ x, float* __restrict__ xt, int64_t n, int d) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const float* xr = x + r * d;
    const float nr = norm_sse_order([&](int i) { return xr[i]; }, d);
    // sqrtf(nr) as the float of the double root (53 bits round to the correctly rounded float root), whatever the compiler's
    // float sqrt is built as
    const float root = (float)sqrt((double)nr);
    const float inv = nr > 0 ? (float)(1.0 / (double)root) : 0.f;
    for (int i = lane; i < d; i += 64) xt[r * d + i] = nr > 0 ? __fmul_rn(xr[i], inv) : xr[i];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

void launch_linear_apply(const LinearArgs& a, const TransformPlan& P, hipStream_t stream) {
    if (a.n <= 0) return;
    if (P.small) {
        const dim3 grid((unsigned)((a.d_out + kRowsCols - 1) / kRowsCols), (unsigned)((a.n + kRowsPerBlock - 1) / kRowsPerBlock));
        hipLaunchKernelGGL(linear_rows_kernel, grid, dim3(256), 0, stream, a);
        return;
    }
    const bool vec_x = a.d_in % 4 == 0 && aligned16(a.x), vec_a = a.d_in % 4 == 0 && aligned16(a.A);
    const dim3 grid((unsigned)((a.n + kStripRows - 1) / kStripRows));
    if (P.resident) {
        ensure_dynamic_lds(reinterpret_cast<const void*>(linear_strip_kernel<true>), P.lds);
        hipLaunchKernelGGL(linear_strip_kernel<true>, grid, dim3(256), P.lds, stream, a, vec_x, vec_a);
    } else {
        ensure_dynamic_lds(reinterpret_cast<const void*>(linear_strip_kernel<false>), P.lds);
        hipLaunchKernelGGL(linear_strip_kernel<false>, grid, dim3(256), P.lds, stream, a, vec_x, vec_a);
    }
}

void launch_transpose(const float* A, float* At, int rows, int cols, hipStream_t stream) {
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, stream, A, At, rows, cols);
}

void launch_remap(const float* x, float* xt, int64_t n, int d_src, int d_dst, const int* map, hipStream_t stream) {
    if (n <= 0) return;
    const int64_t blocks = (n * d_dst + 255) / 256;
    hipLaunchKernelGGL(remap_kernel, dim3((unsigned)std::min<int64_t>(blocks, 1 << 20)), dim3(256), 0, stream, x, xt, n, d_src, d_dst, map);
}

void launch_l2norm(const float* x, float* xt, int64_t n, int d, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(l2norm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, x, xt, n, d);
}

}  // namespace vlq
