// List scan under the inner-product metric: IndexIVFPQ with metric_type = METRIC_INNER_PRODUCT, the IP branch of
// InvertedListScanner (IndexIVFPQ.cpp:540-555, :609-624, :1039-1042).  The reference scans with a max-heap over NEGATED
// inner products, so admission, the (distance, scan position) total order and wave_topk.cuh apply as they do for L2:
//   * the table depends on the query only: sim_table[m][j] = -fvec_inner_product(q_m, pq_centroid[m][j], dsub) (:548-555;
//     ProductQuantizer.cpp:424-436), whatever use_precomputed_table says (:397-401 only warns);
//   * per list only a scalar changes: by residual dis0 = -fvec_inner_product(q, centroid[key], d) (:609-616; the coarse_dis
//     handed in is NOT used), otherwise dis0 = 0 (:579-590);
//   * per code dis = dis0 + tab[0][c0] + ... + tab[M-1][c(M-1)] strictly left to right, admitted if dis < heap top (:786-800);
//   * after the reorder every one of the k values is negated (:1039-1042): rows come out in descending inner product, an
//     unfilled slot is label -1 with distance -FLT_MAX.
//
// One workgroup of four waves per query.  The negated table [M][ksub] is built ONCE in LDS from the transposed codebook
// (pq_cent_t[m][component][j]: consecutive threads read consecutive centroids) and stays there for the whole walk; there is
// no per-(query, list) table row to fetch, so the only stream from memory is the codes.  Thread p computes dis0 of probe p
// (four accumulators over d in fvec_inner_product's order, utils.cpp:509-533: 4 d bytes of centroid per probe).  The query's
// probes are then walked in coarse order; every lane loads one code with the widest load its size allows, the next trip's
// code is requested before the current one is looked up, and (dis, scan position) goes to the wave's running selection.
#include "kernels.h"
#include "scan_common.cuh"
#include "scan16_common.cuh"
#include "sse_order.cuh"
#include "wave_topk.cuh"

namespace vlq {

template <int W> struct IpCode { uint32_t w[W > 0 ? W : 1]; };
// one code of W words, by the widest load the row alignment allows (rows are W * 4 bytes apart)
template <int W>
__device__ __forceinline__ IpCode<W> ip_load(const uint8_t* __restrict__ base, int64_t row) {
    IpCode<W> c;
    if constexpr (W % 4 == 0) {
        const uint4* p = reinterpret_cast<const uint4*>(base) + row * (W / 4);
#pragma unroll
        for (int i = 0; i < W / 4; i++) {
            const uint4 v = p[i];
            c.w[4 * i] = v.x; c.w[4 * i + 1] = v.y; c.w[4 * i + 2] = v.z; c.w[4 * i + 3] = v.w;
        }
    } else if constexpr (W % 2 == 0) {
        const uint2* p = reinterpret_cast<const uint2*>(base) + row * (W / 2);
#pragma unroll
        for (int i = 0; i < W / 2; i++) {
            const uint2 v = p[i];
            c.w[2 * i] = v.x; c.w[2 * i + 1] = v.y;
        }
    } else {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(base) + row * W;
#pragma unroll
        for (int i = 0; i < W; i++) c.w[i] = p[i];
    }
    return c;
}

// W > 0: M = 4 W sub-quantizers of 8 bits (ksub = 256), the engineered shapes; W = 0: any M, any ksub <= 256, one byte per
// index read on its own (the shapes the L2 path hands to the generic scan_kernel).
template <int W, int KPL>
__global__ __launch_bounds__(256) void scan_ip_kernel(ScanArgs a, IpLayout lay) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    float* lut = reinterpret_cast<float*>(smraw);                                  // [M][ksub], later the merge area
    u64* selq = reinterpret_cast<u64*>(smraw + lay.selq);                          // [4][64]
    ProbeMeta pm;
    pm.carve(smraw + lay.meta, a.nprobe);
    float* sq = reinterpret_cast<float*>(smraw + lay.sq);                          // [d] the query

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t q = blockIdx.x;
    const int M = W > 0 ? 4 * W : a.M;
    const int ksub = W > 0 ? 256 : a.ksub;
    const int E = M * ksub;
    const int64_t* kq = a.keys + q * a.nprobe;
    const float* qv = a.queries + q * a.d;

    for (int e = t; e < a.d; e += 256) sq[e] = qv[e];
    const bool badkey = probe_meta_fill(a, q, pm, t, 256);
    __syncthreads();
    // dis0 of every probe (IndexIVFPQ.cpp:609-616 by residual, :579-590 otherwise) in place of the coarse distance
    // probe_meta_fill left there: the scan never reads the caller's coarse_dis
    for (int p = t; p < a.nprobe; p += 256) {
        const int64_t key = kq[p];
        float dis0 = 0.f;
        if (a.table_mode != 2 && key >= 0 && key < a.nlist) {
            const float* c = a.coarse + key * a.d;
            dis0 = -ip_sse_order([&](int i) { return sq[i]; }, [&](int i) { return c[i]; }, a.d);
        }
        pm.pd0[p] = dis0;
    }
    if (wave == 0) probe_meta_scan(a, pm, lane);       // prefix sums, the max_codes cut (IndexIVFPQ.cpp:1033)
    // the negated table, once per query (:548-555)
    for (int e = t; e < E; e += 256) {
        const int m = e / ksub, j = e - m * ksub;
        const float* xm = sq + m * a.dsub;
        const float* ct = a.pq_cent_t + (size_t)m * a.dsub * ksub + j;
        lut[e] = -ip_sse_order([&](int c) { return xm[c]; }, [&](int c) { return ct[(size_t)c * ksub]; }, a.dsub);
    }
    __syncthreads();

    WaveSelect<KPL> sel;
    sel.init(a.k, selq + wave * 64, lane);

    for (int p = 0; p < a.nprobe; p++) {
        if (pm.pkey[p] < 0) continue;                  // (workgroup-uniform) invalid key, empty list, behind the cut
        const uint32_t len = pm.plen[p], pos0 = pm.cum[p];
        const int64_t off = pm.poff[p];
        const float dis0 = pm.pd0[p];
        uint32_t j0 = (uint32_t)wave * 64;
        if (j0 >= len) continue;
        if constexpr (W > 0) {
            IpCode<W> c = ip_load<W>(a.codes, off + min(j0 + lane, len - 1));
            for (; j0 < len; j0 += 256) {
                const uint32_t j = j0 + lane;
                // the next trip's code is on its way while this one is looked up (clamped: never past the list)
                const IpCode<W> cn = ip_load<W>(a.codes, off + min(j + 256, len - 1));
                float dis = dis0;
                const float* tab = lut;
#pragma unroll
                for (int i = 0; i < W; i++) {
                    const uint32_t cw = c.w[i];
                    dis = __fadd_rn(dis, tab[cw & 255u]); tab += 256;
                    dis = __fadd_rn(dis, tab[(cw >> 8) & 255u]); tab += 256;
                    dis = __fadd_rn(dis, tab[(cw >> 16) & 255u]); tab += 256;
                    dis = __fadd_rn(dis, tab[cw >> 24]); tab += 256;
                }
                sel.offer_keyed(dis, pos0 + j, j < len);
                c = cn;
            }
        } else {
            const uint8_t* cp = a.codes + off * M;
            for (; j0 < len; j0 += 256) {
                const uint32_t j = j0 + lane;
                const bool valid = j < len;
                float dis = dis0;
                if (valid) {
                    const uint8_t* cj = cp + (size_t)j * M;
                    const float* tab = lut;
                    for (int m = 0; m < M; m++) { dis = __fadd_rn(dis, tab[cj[m]]); tab += ksub; }
                }
                sel.offer_keyed(dis, pos0 + j, valid);
            }
        }
    }

    const unsigned long long nscan = pm.cum[a.nprobe];
    if (t == 0) atomicAdd(a.ncode, nscan);
    if (badkey) *a.bad_key = 1;                        // (every thread looked at its own probes)
    if (!merge_waves<KPL>(sel, smraw, a.k, wave, lane)) return;
    // rows out: emit_rows (scan_common.cuh) with every value negated, padding included (IndexIVFPQ.cpp:1039-1042)
#pragma unroll
    for (int r = 0; r < KPL; r++) {
        const int e = r * 64 + lane;
        if (e >= a.k) continue;
        const u64 key = sel.best[r];
        float dis = 3.402823466e+38f;          // Heap.h:318-321 padding
        int64_t id = -1;
        if (key != kMaxKey) {
            dis = ordered_to_f32((uint32_t)(key >> 32));
            const uint32_t pos = (uint32_t)key;
            int lo = 0, hi = a.nprobe;         // last probe p with cum[p] <= pos
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (pm.cum[mid] <= pos) lo = mid; else hi = mid;
            }
            const int64_t o = pos - pm.cum[lo];
            id = a.store_pairs ? (kq[lo] << 32 | o) : a.ids[pm.poff[lo] + o];   // IndexIVFPQ.cpp:798
        }
        a.D[q * a.k + e] = -dis;
        a.I[q * a.k + e] = id;
    }
}

template <int W, int KPL>
static bool launch_ip_i(const ScanArgs& a, const IpLayout& lay, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(scan_ip_kernel<W, KPL>), lay.bytes);
    hipLaunchKernelGGL((scan_ip_kernel<W, KPL>), dim3((unsigned)a.nq), dim3(256), lay.bytes, s, a, lay);
    return true;
}
template <int W>
static bool launch_ip_k(const ScanArgs& a, const IpLayout& lay, hipStream_t s) {
    if (a.k <= 64) return launch_ip_i<W, 1>(a, lay, s);
    if (a.k <= 256) return launch_ip_i<W, 4>(a, lay, s);
    return launch_ip_i<W, 16>(a, lay, s);
}

bool launch_scan_ip(const ScanArgs& a, hipStream_t s) {
    if (a.nq <= 0) return true;
    if (!ip_shape_ok(a.M, a.ksub, a.nprobe, a.k, a.d) || (a.table_mode != 1 && a.table_mode != 2)) return false;
    const IpLayout lay = ip_layout(a.M, a.ksub, a.nprobe, a.k, a.d);
    if (ip_engineered(a.M, a.ksub)) {
        switch (a.M / 4) {
#define VLQ_IP(W) case W: return launch_ip_k<W>(a, lay, s)
        VLQ_IP(1); VLQ_IP(2); VLQ_IP(3); VLQ_IP(4); VLQ_IP(5); VLQ_IP(6); VLQ_IP(7); VLQ_IP(8);
        VLQ_IP(9); VLQ_IP(10); VLQ_IP(11); VLQ_IP(12); VLQ_IP(13); VLQ_IP(14); VLQ_IP(15); VLQ_IP(16);
#undef VLQ_IP
        }
    }
    return launch_ip_k<0>(a, lay, s);
}

__global__ void coarse_ip_finish_kernel(float* __restrict__ cdis, const int64_t* __restrict__ keys, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // + 0.0f: an inner product of zero is +0 in the reference (its accumulators start at +0), never -0
    cdis[i] = keys[i] < 0 ? -3.402823466e+38f : __fadd_rn(__fmul_rn(-0.5f, cdis[i]), 0.0f);
}

void launch_coarse_ip_finish(float* cdis, const int64_t* keys, int64_t n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(coarse_ip_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cdis, keys, n);
}

}  // namespace vlq
