// The kernels of the moments handle (include/vlq_ivfpq.h, vlq_moments_*; the launch decision: moments_plan.h): the column means
// and the centred second-moment matrix C = Xc^T Yc that PCAMatrix::train (and the OPQ loop's x^T * pq_recons) spend their time in.
//
// moment_kernel<KR>: a product whose reduction is the LONG dimension.  A workgroup of four waves owns one 128 x 128 tile
// (ta, tb) of C and one slice of rows; the four waves sit 2 x 2 over the tile, each with 2 x 2 accumulators of
// v_mfma_f32_32x32x2_f32 (64 registers) that live for the whole slice and leave the registers once.  The reduction index is the
// ROW, so both MFMA operands are "k-major" in memory already: lane l wants element [row r0 + l / 32][column c0 + l % 32] of its
// panel.  A strip of KR rows of the ta panel and of the tb panel is staged row-major, [KR][128] each, exactly as it lies in HBM
// (one float4 per thread and trip, 512 contiguous bytes per 32 lanes in, one ds_write_b128 out), and every operand read is one
// ds_read_b32 of 32 consecutive floats per half-wave: no transposed or de-interleaved staging, no bank conflict.
//   Centring: one __fsub_rn per component between the global load and the LDS store.  A thread's four columns are the same in
//   every trip (256 threads = 8 rows of 32 float4), so its eight mean components sit in registers for the whole kernel.
//   Padding: rows at or behind the slice's end and columns at or behind d are staged as 0.0f AFTER centring -- a padded row adds
//   nothing, not -mean.
//   Two buffers: strip i + 1 is loaded into registers before the MFMAs of strip i are issued and committed to the other buffer
//   behind them; one barrier a strip.  LDS [2 buffers][2 panels][KR][128] floats.
//   A diagonal pair of the symmetric case stages ONE panel and reads both operands from it.
//   d % 4 != 0 (or an unaligned base) takes scalar loads, as MfmaTile::fetch does with vec_ok.
// moment_reduce_kernel: part[S][pairs][128][128] -> C, every element the sum of its S partials in ascending slice order in double,
// rounded once.  Symmetric: a pair (ta < tb) writes its tile and the mirrored one, a diagonal pair writes from its upper triangle
// only, so C == C^T bit for bit by construction.
// colsum_kernel / colsum_reduce_kernel: the same two stages for the column means.
// No atomics anywhere: the bits depend on (n, dx, dy, the plan) alone.
#include "moments_plan.h"

#include "kernels.h"
#include "mfma_tile.cuh"

namespace vlq {
namespace {

static_assert(kMomTile == 128, "four waves of 2 x 2 accumulators of 32 x 32, 32 float4 per staged row");

// the four columns c .. c + 3 of a mean (NULL: nothing is subtracted), zeros behind d
__device__ __forceinline__ float4 mean4(const float* __restrict__ mean, int c, int d) {
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mean) {
        if (c + 0 < d) m.x = mean[c + 0];
        if (c + 1 < d) m.y = mean[c + 1];
        if (c + 2 < d) m.z = mean[c + 2];
        if (c + 3 < d) m.w = mean[c + 3];
    }
    return m;
}

// KR rows from row0 of the panel at column c0 of x [.][d], centred, into registers: thread t owns columns c0 + 4 (t & 31) .. + 3
// of rows (t >> 5) + 8 i.  Rows at or behind r_end and columns at or behind d: 0.0f.
template <int KR>
__device__ __forceinline__ void fetch_strip(const float* __restrict__ x, int d, int c0, float4 m, bool vec, int64_t row0, int64_t r_end,
                                            float4 (&fr)[KR / 8], int t) {
    const int c = c0 + 4 * (t & 31);
#pragma unroll
    for (int i = 0; i < KR / 8; i++) {
        const int64_t grow = row0 + (t >> 5) + 8 * i;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (grow < r_end && c < d) {
            const float* p = x + grow * d + c;
            if (vec) {                                     // (d % 4 == 0: c < d is c + 4 <= d)
                const float4 g = *reinterpret_cast<const float4*>(p);
                val = make_float4(__fsub_rn(g.x, m.x), __fsub_rn(g.y, m.y), __fsub_rn(g.z, m.z), __fsub_rn(g.w, m.w));
            } else {
                val.x = __fsub_rn(p[0], m.x);
                if (c + 1 < d) val.y = __fsub_rn(p[1], m.y);
                if (c + 2 < d) val.z = __fsub_rn(p[2], m.z);
                if (c + 3 < d) val.w = __fsub_rn(p[3], m.w);
            }
        }
        fr[i] = val;
    }
}

template <int KR>
__device__ __forceinline__ void commit_strip(const float4 (&fr)[KR / 8], float* dst, int t) {
#pragma unroll
    for (int i = 0; i < KR / 8; i++)
        *reinterpret_cast<float4*>(dst + ((t >> 5) + 8 * i) * kMomTile + 4 * (t & 31)) = fr[i];
}

// acc[ti][tj] += sum over the strip's KR rows of sa[row][wr 64 + ti 32 + .] * sb[row][wc 64 + tj 32 + .]: the MFMA takes rows in
// pairs, lane >> 5 picks the row of the pair
template <int KR>
__device__ __forceinline__ void multiply_strip(const float* sa, const float* sb, f32x16 (&acc)[2][2], int t) {
    const int lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1, h = lane >> 5, r = lane & 31;
    const float* pa = sa + h * kMomTile + wr * 64 + r;
    const float* pb = sb + h * kMomTile + wc * 64 + r;
#pragma unroll
    for (int kk = 0; kk < KR / 2; kk++) {
        const float a0 = pa[2 * kk * kMomTile], a1 = pa[2 * kk * kMomTile + 32];
        const float b0 = pb[2 * kk * kMomTile], b1 = pb[2 * kk * kMomTile + 32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}

template <int KR>
__global__ __launch_bounds__(256) void moment_kernel(MomentArgs a, int tiles_x, int pairs, int64_t slice_len, bool vec_x, bool vec_y) {
    extern __shared__ float4 moment_smem[];
    float* sm = reinterpret_cast<float*>(moment_smem);
    constexpr int kPanel = KR * kMomTile;                  // floats of one staged panel
    const int t = threadIdx.x;
    const bool symmetric = a.y == nullptr;
    // the pair: symmetric, the upper triangle row by row (ta <= tb); otherwise the full grid, tb fastest
    int ta, tb;
    if (symmetric) {
        int p = blockIdx.x;
        ta = 0;
        while (p >= tiles_x - ta) { p -= tiles_x - ta; ta++; }
        tb = ta + p;
    } else {
        const int tiles_y = pairs / tiles_x;
        ta = blockIdx.x / tiles_y;
        tb = blockIdx.x % tiles_y;
    }
    const bool diag = symmetric && ta == tb;
    const float* xb = symmetric ? a.x : a.y;
    const int db = symmetric ? a.dx : a.dy;
    const bool vec_b = symmetric ? vec_x : vec_y;
    const float4 ma = mean4(a.mean_x, ta * kMomTile + 4 * (t & 31), a.dx);
    const float4 mb = mean4(symmetric ? a.mean_x : a.mean_y, tb * kMomTile + 4 * (t & 31), db);

    const int64_t r_begin = (int64_t)blockIdx.y * slice_len;
    const int64_t r_end = r_begin + slice_len < a.n ? r_begin + slice_len : a.n;
    const int nstrips = r_begin < r_end ? (int)((r_end - r_begin + KR - 1) / KR) : 0;

    // the accumulators: the partial of the pages before this one, or zeros
    const int lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1, h = lane >> 5, r = lane & 31;
    float* part = a.part + ((size_t)blockIdx.y * pairs + blockIdx.x) * kMomTileFloats;
    f32x16 acc[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int i = wr * 64 + ti * 32 + (e & 3) + 8 * (e >> 2) + 4 * h, j = wc * 64 + tj * 32 + r;
                acc[ti][tj][e] = a.carry ? part[i * kMomTile + j] : 0.f;
            }

    float4 fa[KR / 8], fb[KR / 8];
    if (nstrips > 0) {
        fetch_strip<KR>(a.x, a.dx, ta * kMomTile, ma, vec_x, r_begin, r_end, fa, t);
        if (!diag) fetch_strip<KR>(xb, db, tb * kMomTile, mb, vec_b, r_begin, r_end, fb, t);
        commit_strip<KR>(fa, sm, t);
        if (!diag) commit_strip<KR>(fb, sm + kPanel, t);
    }
    __syncthreads();
    for (int it = 0; it < nstrips; it++) {
        float* cur = sm + (it & 1) * 2 * kPanel;
        float* nxt = sm + ((it + 1) & 1) * 2 * kPanel;
        const bool more = it + 1 < nstrips;
        if (more) {
            const int64_t row0 = r_begin + (int64_t)(it + 1) * KR;
            fetch_strip<KR>(a.x, a.dx, ta * kMomTile, ma, vec_x, row0, r_end, fa, t);
            if (!diag) fetch_strip<KR>(xb, db, tb * kMomTile, mb, vec_b, row0, r_end, fb, t);
        }
        multiply_strip<KR>(cur, diag ? cur : cur + kPanel, acc, t);
        if (more) {
            // nxt was last read in strip it - 1, and every wave has passed that strip's barrier
            commit_strip<KR>(fa, nxt, t);
            if (!diag) commit_strip<KR>(fb, nxt + kPanel, t);
        }
        __syncthreads();
    }

    // C/D layout of an accumulator: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5): a half-wave stores 128
    // contiguous bytes
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int i = wr * 64 + ti * 32 + (e & 3) + 8 * (e >> 2) + 4 * h, j = wc * 64 + tj * 32 + r;
                part[i * kMomTile + j] = acc[ti][tj][e];
            }
}

// grid (pairs, 64): a thread joins one element of a pair's tile; eight partials are in flight at a time, added in order
__global__ __launch_bounds__(256) void moment_reduce_kernel(const float* __restrict__ part, int S, int pairs, int tiles_x, int dx, int dy,
                                                            bool symmetric, float* __restrict__ C) {
    int ta, tb;
    if (symmetric) {
        int p = blockIdx.x;
        ta = 0;
        while (p >= tiles_x - ta) { p -= tiles_x - ta; ta++; }
        tb = ta + p;
    } else {
        const int tiles_y = pairs / tiles_x;
        ta = blockIdx.x / tiles_y;
        tb = blockIdx.x % tiles_y;
    }
    const int idx = blockIdx.y * 256 + threadIdx.x;
    const int i = idx / kMomTile, j = idx % kMomTile;
    const int ca = ta * kMomTile + i, cb = tb * kMomTile + j;
    if (ca >= dx || cb >= dy) return;
    if (symmetric && ta == tb && i > j) return;                    // a diagonal tile: the upper triangle speaks for both
    const float* p = part + (size_t)blockIdx.x * kMomTileFloats + idx;
    const size_t stride = (size_t)pairs * kMomTileFloats;
    double sum = 0.0;
    int s = 0;
    for (; s + 8 <= S; s += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = p[(size_t)(s + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; u++) sum += (double)v[u];
    }
    for (; s < S; s++) sum += (double)p[(size_t)s * stride];
    const float v = (float)sum;
    C[(size_t)ca * dy + cb] = v;
    if (symmetric) C[(size_t)cb * dy + ca] = v;
}

// grid (ceil(d / 64), col_slices): thread (c = t & 63, q = t >> 6) adds rows q, q + 4, .. of the slice for column c in fp32; the
// four row lanes are joined in LDS in the order q = 0 .. 3
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, int64_t n, int d, int64_t slice_len, bool carry,
                                                     float* __restrict__ part) {
    __shared__ float red[kColLanes][kColCols];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int j = blockIdx.x * kColCols + c;
    const int64_t r_begin = (int64_t)blockIdx.y * slice_len;
    const int64_t r_end = r_begin + slice_len < n ? r_begin + slice_len : n;
    float acc = 0.f;
    if (j < d) {
#pragma unroll 4
        for (int64_t row = r_begin + q; row < r_end; row += kColLanes) acc = __fadd_rn(acc, x[row * d + j]);
    }
    red[q][c] = acc;
    __syncthreads();
    if (q == 0 && j < d) {
        float sum = red[0][c];
#pragma unroll
        for (int u = 1; u < kColLanes; u++) sum = __fadd_rn(sum, red[u][c]);
        float* dst = part + (size_t)blockIdx.y * d + j;
        if (!carry) *dst = sum;
        else if (r_begin < r_end) *dst = __fadd_rn(*dst, sum);
    }
}

// grid (ceil(d / 16)): thread (c = t & 15, q = t >> 4) adds the q-th sixteenth of the slices of column c in ascending order in
// double; the sixteen chunk sums are added in ascending order, then the one division
__global__ __launch_bounds__(256) void colsum_reduce_kernel(const float* __restrict__ part, int slices, int d, int64_t n_total,
                                                            float* __restrict__ mean) {
    __shared__ double red[16][16];
    const int c = threadIdx.x & 15, q = threadIdx.x >> 4;
    const int j = blockIdx.x * 16 + c;
    const int chunk = (slices + 15) / 16;
    const int s_end = (q + 1) * chunk < slices ? (q + 1) * chunk : slices;
    double sum = 0.0;
    if (j < d) {
#pragma unroll 8
        for (int s = q * chunk; s < s_end; s++) sum += (double)part[(size_t)s * d + j];
    }
    red[q][c] = sum;
    __syncthreads();
    if (q == 0 && j < d) {
        double total = red[0][c];
#pragma unroll
        for (int u = 1; u < 16; u++) total += red[u][c];
        mean[j] = (float)(total / (double)n_total);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int KR>
void launch_moment_kr(const MomentArgs& a, const MomentsPlan& P, hipStream_t stream) {
    const bool vec_x = a.dx % 4 == 0 && aligned16(a.x), vec_y = a.y && a.dy % 4 == 0 && aligned16(a.y);
    ensure_dynamic_lds(reinterpret_cast<const void*>(moment_kernel<KR>), P.lds);
    hipLaunchKernelGGL(moment_kernel<KR>, dim3((unsigned)P.pairs, (unsigned)P.S), dim3(256), P.lds, stream, a, P.tiles_x, P.pairs, P.slice_len,
                       vec_x, vec_y);
}

}  // namespace

void launch_colsum(const float* x, int64_t n, int d, const MomentsPlan& P, bool carry, float* part, hipStream_t stream) {
    const dim3 grid((unsigned)((d + kColCols - 1) / kColCols), (unsigned)P.col_slices);
    hipLaunchKernelGGL(colsum_kernel, grid, dim3(256), 0, stream, x, n, d, P.col_slice_len, carry, part);
}

void launch_colsum_reduce(const float* part, int slices, int d, int64_t n_total, float* mean, hipStream_t stream) {
    hipLaunchKernelGGL(colsum_reduce_kernel, dim3((unsigned)((d + 15) / 16)), dim3(256), 0, stream, part, slices, d, n_total, mean);
}

void launch_moment(const MomentArgs& a, const MomentsPlan& P, hipStream_t stream) {
    if (P.kr == 16) launch_moment_kr<16>(a, P, stream);
    else if (P.kr == 64) launch_moment_kr<64>(a, P, stream);
    else launch_moment_kr<32>(a, P, stream);
}

void launch_moment_reduce(const float* part, const MomentsPlan& P, int dx, int dy, bool symmetric, float* C, hipStream_t stream) {
    hipLaunchKernelGGL(moment_reduce_kernel, dim3((unsigned)P.pairs, 64), dim3(256), 0, stream, part, P.S, P.pairs, P.tiles_x, dx, dy, symmetric, C);
}

}  // namespace vlq
