// Rows out of (distance, position) keys, shared by the exhaustive scans (scan_pq.hip, scan_knn.hip): the emit of a finished
// selection and the join of the partial rows that the slices of one query left in scratch.  The key order is total, so the
// joined row depends on no slicing.
#pragma once
#include "wave_topk.cuh"

namespace vlq {

__device__ __forceinline__ float flip_sign(float v, uint32_t neg) { return __uint_as_float(__float_as_uint(v) ^ neg); }

// rows out of a finished selection: (distance, position), padded FLT_MAX / -1 (Heap.h:318-321); neg = 0x80000000 under inner product
template <int KPL, typename Sel>
__device__ __forceinline__ void pq_emit(const Sel& sel, int k, uint32_t neg, float* __restrict__ D, int64_t* __restrict__ I, int lane) {
#pragma unroll
    for (int r = 0; r < KPL; r++) {
        const int e = r * 64 + lane;
        if (e >= k) continue;
        const u64 key = sel.best[r];
        float dis = 3.402823466e+38f;
        int64_t id = -1;
        if (key != kMaxKey) { dis = ordered_to_f32((uint32_t)(key >> 32)); id = (int64_t)(uint32_t)key; }
        D[e] = flip_sign(dis, neg);
        I[e] = id;
    }
}

// the S slices' keys of a query -> its row; one wave per query.  The keys of query q start at part + q * stride (S * k of them
// are read).  keys_out == nullptr: the row goes to D / I; otherwise the joined k keys go to keys_out + q * out_stride (a running
// row that a later join takes as one more slice; it may lie inside the query's own `part` rows: everything is read before
// anything is written) and D / I are not touched.
template <int KPL>
__global__ __launch_bounds__(256) void pq_join_kernel(const u64* part, int64_t nq, int S, int64_t stride, int k, uint32_t neg,
                                                      float* __restrict__ D, int64_t* __restrict__ I, u64* keys_out, int64_t out_stride) {
    __shared__ u64 queue[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t q = (int64_t)blockIdx.x * 4 + wave;
    if (q >= nq) return;
    WaveSelect<KPL> sel;
    sel.init(k, queue[wave], lane);
    const u64* rows = part + (size_t)q * stride;
    for (int s = 0; s < S; s++)
        for (int e0 = 0; e0 < k; e0 += 64) {
            const int e = e0 + lane;
            const bool valid = e < k;
            sel.offer_key(valid ? rows[(size_t)s * k + e] : kMaxKey, valid);
        }
    sel.flush();
    if (keys_out) {
        u64* out = keys_out + (size_t)q * out_stride;
#pragma unroll
        for (int r = 0; r < KPL; r++) {
            const int e = r * 64 + lane;
            if (e < k) out[e] = sel.best[r];
        }
    } else {
        pq_emit<KPL>(sel, k, neg, D + q * k, I + q * k, lane);
    }
}

// kpl: 1 (k <= 64), 4 (k <= 256), 16 (k <= 1024)
inline void launch_join_rows(int kpl, const u64* part, int64_t nq, int S, int64_t stride, int k, uint32_t neg, float* D, int64_t* I,
                             u64* keys_out, int64_t out_stride, hipStream_t s) {
    if (nq <= 0) return;
    const dim3 grid((unsigned)((nq + 3) / 4));
    if (kpl == 1) hipLaunchKernelGGL(pq_join_kernel<1>, grid, dim3(256), 0, s, part, nq, S, stride, k, neg, D, I, keys_out, out_stride);
    else if (kpl == 4) hipLaunchKernelGGL(pq_join_kernel<4>, grid, dim3(256), 0, s, part, nq, S, stride, k, neg, D, I, keys_out, out_stride);
    else hipLaunchKernelGGL(pq_join_kernel<16>, grid, dim3(256), 0, s, part, nq, S, stride, k, neg, D, I, keys_out, out_stride);
}

}  // namespace vlq
