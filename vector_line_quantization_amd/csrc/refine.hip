// IVFPQR: the re-ranking stage of IndexIVFPQR::search (IndexIVFPQ.cpp:1392-1444) and the second-level residuals of
// IndexIVFPQR::add_core (:1341-1357, IndexIVFPQ.cpp:250-256) on the device.
//
// Per shortlist entry (list << 32 | offset, -1 = skip), in shortlist order:
//   r1 = x - coarse[list]                      Index::compute_residual, Index.cpp:76-81
//   r2 = r1 - pq.decode(codes[list][ofs])      ProductQuantizer.cpp:338-352
//   r3 = refine_pq.decode(refine code)         (stored by list slot, beside the PQ code)
//   dis = fvec_L2sqr(r3, r2, d)                utils.cpp:481-506 -- l2sqr_sse_order, never fused
// and the k smallest (dis, shortlist position) of a query, ascending, padded with -1 / FLT_MAX.
//
// Mapping: one wave per query, one lane per shortlist entry with the four SSE accumulators of its own -- a candidate
// is four independent serial chains of d / 4 steps, 64 candidates in flight per wave hide the gathers of their
// sub-centroid rows (both tables and the coarse centroids stay in L2: they are shared by every query).  The query row
// sits in LDS, read by all lanes at one address (a broadcast).  The selection is wave_topk.cuh's with the shortlist
// position as the key's low word; candidates are offered in increasing position, so its strict admission is the
// reference's `dis < heap_sim[0]`.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "sse_order.cuh"
#include "wave_topk.cuh"

namespace vlq {

namespace {

constexpr float kFltMax = 3.402823466e+38f;

// decoded PQ vector read in ascending dimension order, one sub-centroid row after the other.  VEC (dsub % 4 == 0,
// 16-byte aligned rows): a row is fetched four floats at a time, at the dimensions that are multiples of four.
template <bool VEC>
struct DecodeWalk {
    const float* cent;       // [M][ksub][dsub]
    const uint8_t* code;     // [M]
    int ksub, dsub, m, off;
    const float* row;
    float4 v;
    __device__ __forceinline__ void init(const float* cent_, const uint8_t* code_, int ksub_, int dsub_) {
        cent = cent_; code = code_; ksub = ksub_; dsub = dsub_;
        m = 0; off = 0;
        row = cent + (size_t)(code[0] & (ksub - 1)) * dsub;     // (a byte past ksub cannot leave the table)
    }
    __device__ __forceinline__ void step() {
        if (off == dsub) {
            m++; off = 0;
            row = cent + ((size_t)m * ksub + (code[m] & (ksub - 1))) * dsub;
        }
    }
    // i ascends by one from 0 over the calls
    __device__ __forceinline__ float get(int i) {
        if (VEC) {
            if ((i & 3) == 0) { step(); v = *reinterpret_cast<const float4*>(row + off); off += 4; }
            const int c = i & 3;
            return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w;
        }
        step();
        return row[off++];
    }
};

// x - coarse centroid in ascending dimension order
template <bool VEC>
struct ResidualWalk {
    const float* x;          // LDS
    const float* c;
    float4 xv, cv;
    __device__ __forceinline__ float get(int i) {
        if (VEC) {
            if ((i & 3) == 0) { xv = *reinterpret_cast<const float4*>(x + i); cv = *reinterpret_cast<const float4*>(c + i); }
            const int e = i & 3;
            const float a = e == 0 ? xv.x : e == 1 ? xv.y : e == 2 ? xv.z : xv.w;
            const float b = e == 0 ? cv.x : e == 1 ? cv.y : e == 2 ? cv.z : cv.w;
            return __fsub_rn(a, b);
        }
        return __fsub_rn(x[i], c[i]);
    }
};

// slot of a pair label in the flat list arrays, or -1 when the pair lies outside the lists
__device__ __forceinline__ int64_t pair_slot(int64_t sl, int nlist, const int64_t* __restrict__ list_off,
                                             const int64_t* __restrict__ list_len) {
    const int64_t list = sl >> 32;
    const int64_t ofs = sl & 0xffffffffll;
    if (list < 0 || list >= nlist) return -1;
    if (ofs >= list_len[list]) return -1;
    return list_off[list] + ofs;
}

template <int KPL, bool VEC>
__global__ __launch_bounds__(256) void refine_kernel(RefineArgs a) {
    __shared__ u64 queue[4][64];
    extern __shared__ __attribute__((aligned(16))) float xs[];   // [4][d]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + wave;
    if (q >= a.nq) return;                                       // (wave-uniform; no workgroup barrier below)
    const int d = a.d;
    float* x = xs + wave * d;
    for (int c = lane; c < d; c += 64) x[c] = a.x[q * d + c];
    __builtin_amdgcn_wave_barrier();
    const int64_t* sl_row = a.shortlist + q * a.k_coarse;
    WaveSelect<KPL> sel;
    sel.init(a.k, queue[wave], lane);
    for (int j0 = 0; j0 < a.k_coarse; j0 += 64) {
        const int j = j0 + lane;
        bool valid = j < a.k_coarse;
        const int64_t sl = valid ? sl_row[j] : -1;
        valid = valid && sl != -1;                               // IndexIVFPQ.cpp:1411
        float dis = 0.f;
        if (valid) {
            const int64_t slot = pair_slot(sl, a.nlist, a.list_off, a.list_len);
            if (slot < 0) {                                      // the reference asserts (:1416-1417)
                *a.bad = 4;
                valid = false;
            } else {
                ResidualWalk<VEC> r1;
                r1.x = x; r1.c = a.coarse + (sl >> 32) * d;
                DecodeWalk<VEC> p, r3;
                p.init(a.pq, a.codes + slot * a.M, a.ksub, a.dsub);
                r3.init(a.rpq, a.rcodes + slot * a.Mr, a.ksub_r, a.dsub_r);
                // fvec_L2sqr (residual_1 = r3, residual_2 = r2, d), IndexIVFPQ.cpp:1434; the helper asks for x(i), y(i) with
                // i ascending, which is what the walkers serve
                dis = l2sqr_sse_order([&](int i) { return r3.get(i); },
                                      [&](int i) { return __fsub_rn(r1.get(i), p.get(i)); }, d);
            }
        }
        sel.offer(dis, (uint32_t)j, valid);
    }
    sel.flush();
#pragma unroll
    for (int r = 0; r < KPL; r++) {
        const int e = r * 64 + lane;
        if (e >= a.k) continue;
        const u64 key = sel.best[r];
        float dis = kFltMax;
        int64_t id = -1;
        if (key != kMaxKey) {
            dis = ordered_to_f32((uint32_t)(key >> 32));
            id = a.ids[pair_slot(sl_row[(uint32_t)key], a.nlist, a.list_off, a.list_len)];    // (admitted: the slot is valid)
        }
        a.D[q * a.k + e] = dis;
        a.I[q * a.k + e] = id;
    }
}

// r2 of the vectors of an add batch: (x - coarse[assign]) - pq.decode(code), IndexIVFPQ.cpp:250-256 (a vector without a
// list is dropped by the append; its row is zero)
__global__ void residual2_kernel(const float* __restrict__ x, int64_t n, int d, const float* __restrict__ coarse,
                                 const int64_t* __restrict__ assign, const float* __restrict__ pq, const uint8_t* __restrict__ codes,
                                 int M, int ksub, int dsub, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * d) return;
    const int64_t v = e / d;
    const int c = (int)(e - v * d);
    const int64_t key = assign[v];
    float r = 0.f;
    if (key >= 0) {
        const int m = c / dsub;
        const float r1 = __fsub_rn(x[e], coarse[key * d + c]);
        r = __fsub_rn(r1, pq[((size_t)m * ksub + codes[v * M + m]) * dsub + (c - m * dsub)]);
    }
    out[e] = r;
}

template <int KPL>
void launch_refine_t(const RefineArgs& a, bool vec, hipStream_t s) {
    const dim3 grid((unsigned)((a.nq + 3) / 4)), block(256);
    const size_t smem = (size_t)4 * a.d * sizeof(float);
    if (vec) hipLaunchKernelGGL((refine_kernel<KPL, true>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((refine_kernel<KPL, false>), grid, block, smem, s, a);
}

}  // namespace

void launch_refine(const RefineArgs& a, hipStream_t s) {
    if (a.nq <= 0) return;
    const bool vec = a.d % 4 == 0 && a.dsub % 4 == 0 && a.dsub_r % 4 == 0;
    if (a.k <= 64) launch_refine_t<1>(a, vec, s);
    else if (a.k <= 256) launch_refine_t<4>(a, vec, s);
    else if (a.k <= 512) launch_refine_t<8>(a, vec, s);
    else launch_refine_t<16>(a, vec, s);
}

void launch_residual2(const float* x, int64_t n, int d, const float* coarse, const int64_t* assign, const float* pq,
                      const uint8_t* codes, int M, int ksub, int dsub, float* out, hipStream_t s) {
    if (n <= 0) return;
    const int64_t e = n * d;
    hipLaunchKernelGGL(residual2_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, x, n, d, coarse, assign, pq, codes,
                       M, ksub, dsub, out);
}

}  // namespace vlq
