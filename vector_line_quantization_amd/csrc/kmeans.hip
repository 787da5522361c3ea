// k-means on the device: what one Lloyd iteration needs after the assignment (scan_knn.hip at k = 1 does that half).
//   km_update_centroids   utils.cpp:1369-1450   -> kmeans_key_kernel + radix sort + kmeans_bounds_kernel (grouping),
//                                                  kmeans_update_kernel / kmeans_update_packed_kernel (the ordered sums and
//                                                  the division), kmeans_split_kernel (the rows of the host's splits)
//   fvec_renorm_L2        utils.cpp:686-701     -> kmeans_renorm_kernel
//   x[perm[i]]            Clustering.cpp:86-91, :137-141 -> kmeans_gather_kernel
//   err += dis[j]         Clustering.cpp:166-168 -> kmeans_objective_kernel (in double, a fixed order: NOT the reference's chain)
// The sums are the reference's bit for bit: for every (centroid, component) one left-to-right fp32 chain from 0.0f over the
// centroid's rows in ascending row order.  Nothing here may reassociate: no fast-math, no pairwise sums, no wider accumulator.
// kmeans_plan.h has the split of the work.
#include "kmeans_plan.h"
#include "sse_order.cuh"

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

namespace vlq {
namespace {

// ---- grouping ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kmeans_key_kernel(const int64_t* __restrict__ assign, int64_t n, int64_t k, int row_bits,
                                                         unsigned long long* __restrict__ keys, KMeansStatus* status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t a = assign[i];
    const bool bad = a < 0 || a >= k;
    if (bad) status->bad_label = 1;
    keys[i] = ((unsigned long long)(bad ? 0 : a) << row_bits) | (unsigned long long)i;
}

// sorted keys -> rows[p] = the row of place p; start[c] = the first place whose centroid is >= c (thread p writes the starts
// of the centroids that begin between places p - 1 and p: the empty ones in front of its own among them), start[k] = n
__global__ __launch_bounds__(256) void kmeans_bounds_kernel(const unsigned long long* __restrict__ keys, int64_t n, int64_t k, int row_bits,
                                                            uint32_t* __restrict__ rows, int64_t* __restrict__ start) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    const int64_t prev = p == 0 ? -1 : (int64_t)(keys[p - 1] >> row_bits);
    int64_t cur = k;
    if (p < n) {
        const unsigned long long key = keys[p];
        cur = (int64_t)(key >> row_bits);
        rows[p] = (uint32_t)(key & ((1ull << row_bits) - 1));
    }
    for (int64_t c = prev + 1; c <= cur; c++) start[c] = p;
}

// ---- the ordered update -------------------------------------------------------------------------------------------------------
// grid (k, slices / waves): the workgroup's waves own consecutive 64-component slices of centroid blockIdx.x.  Every batch of
// kIdBatch row ids is read once by the workgroup, coalesced, into LDS; a wave then reads an id as a broadcast and fetches
// 64 consecutive floats of that row.  kUnroll loads are issued before the first of their adds: the loads do not depend on the
// chain, the adds keep its order.
__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ x, const uint32_t* __restrict__ rows,
                                                            const int64_t* __restrict__ start, float* __restrict__ cent,
                                                            int64_t* __restrict__ count, KMeansStatus* status, int d) {
    __shared__ uint32_t ids[kIdBatch];
    const int64_t c = blockIdx.x;
    const int nw = (int)blockDim.x >> 6;
    const int j = ((int)blockIdx.y * nw + ((int)threadIdx.x >> 6)) * 64 + ((int)threadIdx.x & 63);
    const bool live = j < d;
    const int64_t s0 = start[c], s1 = start[c + 1];
    const float* xj = x + (live ? j : 0);
    float acc = 0.f;
    for (int64_t b = s0; b < s1; b += kIdBatch) {
        const int nb = (int)(s1 - b < kIdBatch ? s1 - b : kIdBatch);
        __syncthreads();          // the batch before this one has been consumed
        for (int t = threadIdx.x; t < nb; t += blockDim.x) ids[t] = rows[b + t];
        __syncthreads();
        if (!live) continue;
        int t = 0;
        for (; t + kUnroll <= nb; t += kUnroll) {
            float v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) v[u] = xj[(size_t)ids[t + u] * (size_t)d];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) acc = __fadd_rn(acc, v[u]);
        }
        for (; t < nb; t++) acc = __fadd_rn(acc, xj[(size_t)ids[t] * (size_t)d]);
    }
    const int64_t cnt = s1 - s0;
    if (live) cent[(size_t)c * d + j] = cnt ? __fdiv_rn(acc, (float)cnt) : 0.f;
    if (j == 0) {
        count[c] = cnt;
        if (!cnt) status->any_empty = 1;
    }
}

// d < 64: lane g owns (c, j) = (g / d, g % d); the lanes of one centroid read the same id (one address) and d consecutive floats
__global__ __launch_bounds__(256) void kmeans_update_packed_kernel(const float* __restrict__ x, const uint32_t* __restrict__ rows,
                                                                   const int64_t* __restrict__ start, float* __restrict__ cent,
                                                                   int64_t* __restrict__ count, KMeansStatus* status, int64_t k, int d) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= k * d) return;
    const int64_t c = g / d;
    const int j = (int)(g - c * d);
    const int64_t s0 = start[c], s1 = start[c + 1];
    const float* xj = x + j;
    float acc = 0.f;
    int64_t p = s0;
    for (; p + kUnroll <= s1; p += kUnroll) {
        float v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) v[u] = xj[(size_t)rows[p + u] * (size_t)d];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) acc = __fadd_rn(acc, v[u]);
    }
    for (; p < s1; p++) acc = __fadd_rn(acc, xj[(size_t)rows[p] * (size_t)d]);
    const int64_t cnt = s1 - s0;
    cent[g] = cnt ? __fdiv_rn(acc, (float)cnt) : 0.f;
    if (j == 0) {
        count[c] = cnt;
        if (!cnt) status->any_empty = 1;
    }
}

// the splits in the host's order; a thread owns component j through all of them, so a split that copies a row an earlier one
// wrote reads what that one left.  c *= 1 +- EPS with EPS = 1 / 1024. a double: the product in double, rounded to float
__global__ __launch_bounds__(256) void kmeans_split_kernel(float* cent, int d, const int* __restrict__ pairs, int nsplit) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= d) return;
    const double eps = 1 / 1024.;
    const double up = j % 2 == 0 ? 1 + eps : 1 - eps, down = j % 2 == 0 ? 1 - eps : 1 + eps;
    for (int s = 0; s < nsplit; s++) {
        const size_t ci = (size_t)pairs[2 * s], cj = (size_t)pairs[2 * s + 1];
        const float v = cent[cj * d + j];
        cent[ci * d + j] = (float)((double)v * up);
        cent[cj * d + j] = (float)((double)v * down);
    }
}

// ---- the small kernels around it ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kmeans_gather_kernel(const float* __restrict__ x, const int* __restrict__ perm, int64_t m, int d,
                                                            float* __restrict__ out) {
    const int64_t total = m * d, step = (int64_t)gridDim.x * 256;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < total; f += step) {
        const int64_t i = f / d;
        out[f] = x[(size_t)perm[i] * d + (f - i * d)];
    }
}

// fvec_renorm_L2 in place, a wave per row: every lane runs the norm's four chains over the row (one address per load), then
// the lanes share the components.  inv_nr = (float)(1.0 / sqrtf(nr)), the root taken as the float of the double root
__global__ __launch_bounds__(256) void kmeans_renorm_kernel(float* c, int64_t k, int d) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= k) return;
    float* cr = c + r * d;
    const float nr = norm_sse_order([&](int i) { return cr[i]; }, d);
    if (!(nr > 0)) return;
    const float root = (float)sqrt((double)nr);
    const float inv = (float)(1.0 / (double)root);
    for (int i = threadIdx.x & 63; i < d; i += 64) cr[i] = __fmul_rn(cr[i], inv);
}

__device__ double block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(256) void kmeans_objective_kernel(const float* __restrict__ dis, int64_t n, double* __restrict__ partial) {
    __shared__ double sh[256];
    double s = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kObjBlocks * 256) s += (double)dis[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void kmeans_objective_end_kernel(const double* __restrict__ partial, KMeansStatus* status) {
    __shared__ double sh[256];
    const double s = block_sum((int)threadIdx.x < kObjBlocks ? partial[threadIdx.x] : 0.0, sh);
    if (threadIdx.x == 0) status->obj = s;
}

// the same two trees over each of M contiguous rows of n distances (pq_train_api.hip: a slice's objective is kmeans_objective's bits)
__global__ __launch_bounds__(256) void kmeans_objective_batch_kernel(const float* __restrict__ dis, int64_t n, double* __restrict__ partial) {
    __shared__ double sh[256];
    const float* row = dis + (size_t)blockIdx.y * n;
    double s = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kObjBlocks * 256) s += (double)row[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * kObjBlocks + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void kmeans_objective_batch_end_kernel(const double* __restrict__ partial, double* __restrict__ obj) {
    __shared__ double sh[256];
    const double s = block_sum((int)threadIdx.x < kObjBlocks ? partial[(size_t)blockIdx.x * kObjBlocks + threadIdx.x] : 0.0, sh);
    if (threadIdx.x == 0) obj[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void kmeans_finite_kernel(const float* __restrict__ x, int64_t total, KMeansStatus* status) {
    const int64_t step = (int64_t)gridDim.x * 256;
    bool bad = false;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < total; f += step) bad |= !isfinite(x[f]);
    if (bad) status->not_finite = 1;
}

__global__ void kmeans_clear_kernel(KMeansStatus* status) {
    status->bad_label = 0; status->any_empty = 0; status->not_finite = 0; status->pad = 0; status->obj = 0;
}

unsigned blocks_for(int64_t total) { return (unsigned)std::min<int64_t>((total + 255) / 256, 1 << 20); }

}  // namespace

size_t kmeans_sort_bytes(int64_t n, const KMeansPlan& P) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_keys(nullptr, bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)n, 0, (unsigned)P.key_bits,
                                   (hipStream_t)0);
    return bytes;
}

hipError_t launch_kmeans_group(const KMeansGroupArgs& a, const KMeansPlan& P, hipStream_t stream) {
    hipLaunchKernelGGL(kmeans_key_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a.assign, a.n, a.k, P.key_row_bits, a.keys_in,
                       a.status);
    size_t bytes = a.sort_bytes;
    const hipError_t e = rocprim::radix_sort_keys(a.sort_tmp, bytes, a.keys_in, a.keys_out, (size_t)a.n, 0, (unsigned)P.key_bits, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kmeans_bounds_kernel, dim3((unsigned)((a.n + 1 + 255) / 256)), dim3(256), 0, stream, a.keys_out, a.n, a.k, P.key_row_bits,
                       a.rows, a.start);
    return hipGetLastError();
}

void launch_kmeans_update(const float* x, const uint32_t* rows, const int64_t* start, float* cent, int64_t* count, KMeansStatus* status,
                          int64_t k, int d, const KMeansPlan& P, hipStream_t stream) {
    if (P.packed)
        hipLaunchKernelGGL(kmeans_update_packed_kernel, P.grid, dim3(256), 0, stream, x, rows, start, cent, count, status, k, d);
    else
        hipLaunchKernelGGL(kmeans_update_kernel, P.grid, dim3((unsigned)P.waves * 64), 0, stream, x, rows, start, cent, count, status, d);
}

void launch_kmeans_split(float* cent, int d, const int* pairs, int nsplit, hipStream_t stream) {
    if (nsplit <= 0) return;
    hipLaunchKernelGGL(kmeans_split_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, stream, cent, d, pairs, nsplit);
}

void launch_kmeans_gather(const float* x, const int* perm, int64_t m, int d, float* out, hipStream_t stream) {
    if (m <= 0) return;
    hipLaunchKernelGGL(kmeans_gather_kernel, dim3(blocks_for(m * d)), dim3(256), 0, stream, x, perm, m, d, out);
}

void launch_kmeans_renorm(float* c, int64_t k, int d, hipStream_t stream) {
    hipLaunchKernelGGL(kmeans_renorm_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, stream, c, k, d);
}

void launch_kmeans_objective(const float* dis, int64_t n, double* partial, KMeansStatus* status, hipStream_t stream) {
    hipLaunchKernelGGL(kmeans_objective_kernel, dim3(kObjBlocks), dim3(256), 0, stream, dis, n, partial);
    hipLaunchKernelGGL(kmeans_objective_end_kernel, dim3(1), dim3(256), 0, stream, partial, status);
}

void launch_kmeans_objective_batch(const float* dis, int64_t n, int M, double* partial, double* obj, hipStream_t stream) {
    hipLaunchKernelGGL(kmeans_objective_batch_kernel, dim3(kObjBlocks, (unsigned)M), dim3(256), 0, stream, dis, n, partial);
    hipLaunchKernelGGL(kmeans_objective_batch_end_kernel, dim3((unsigned)M), dim3(256), 0, stream, partial, obj);
}

void launch_kmeans_finite(const float* x, int64_t total, KMeansStatus* status, hipStream_t stream) {
    if (total <= 0) return;
    hipLaunchKernelGGL(kmeans_finite_kernel, dim3(blocks_for(total)), dim3(256), 0, stream, x, total, status);
}

void launch_kmeans_clear(KMeansStatus* status, hipStream_t stream) { hipLaunchKernelGGL(kmeans_clear_kernel, dim3(1), dim3(1), 0, stream, status); }

}  // namespace vlq
