// List scan with polysemous Hamming filtering: IndexIVFPQ::polysemous_ht > 0, scan_list_polysemous_hc
// (IndexIVFPQ.cpp:887-947, called at :1023-1025).  A stored code pays for the table look-ups and the selection only if the
// Hamming distance between it and the code of the query is below the threshold (`hd < ht`, :901); hd is the population
// count of q_code XOR code over the whole code -- HammingComputer{4,8,16,20,32,64}, M8 and M4 of hamming.h all give that
// number, so there is one rule here.  Codes that pass get the arithmetic of scan_list_with_table (:781-802): dis0 +
// tab[0][c0] + ... + tab[M-1][c(M-1)] strictly left to right, admitted by (distance, scan position).
//
// q_code[m] is the FIRST argmin over j of the table tab[m][j] the scan itself reads:
//   * not by_residual: the query's distance table, once per query = pq.compute_code(qi) (:544-545, ProductQuantizer.cpp:311-336);
//   * by_residual, table type 2: per (query, list), what fvec_madd_and_argmin leaves while the list's table is built (:676-683);
//   * by_residual, table type 0 / 1: the same rule on the (query, list) table.  The reference never writes q_code there
//     (:635-644 do not touch it) and filters on the Hamming weight of the stored code; this library does not reproduce that.
//
// One workgroup of four waves per query walks the query's probes in coarse order.  Per list: the table is built in LDS,
// wave w reduces sub-quantizers w, w + 4, ... to their (value, index) minimum across its lanes (lower index wins), the
// list's q_code is read back wave-uniform.  Every lane then loads one code with the widest load its size allows, XORs it
// against q_code and counts bits -- no LDS access.  The passing lanes of a trip (one ballot) are compacted into a ring of
// list offsets in LDS, one ring per wave; whenever 64 are waiting the wave looks a full row of passers up and offers it
// to the running selection (wave_topk.cuh).  The ring is drained at every list boundary, where the table changes.
#include "kernels.h"
#include "scan_common.cuh"
#include "scan16_common.cuh"
#include "sse_order.cuh"
#include "wave_topk.cuh"

namespace vlq {

template <int W> struct PolyCode { uint32_t w[W]; };
// one code of W words, by the widest load the row alignment allows (rows are W * 4 bytes apart)
template <int W>
__device__ __forceinline__ PolyCode<W> poly_load(const uint8_t* __restrict__ base, int64_t row) {
    PolyCode<W> c;
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

constexpr int kPolyRing = 128;      // slots of a wave's passer ring: fewer than 64 waiting + at most 64 of one trip

// a.table_mode: 0 by_residual without the precomputed table, 1 by_residual with it (flat or, a.imi_nbits > 0, table type 2),
// 2 not by_residual; read at run time, since it only steers the table build, once per list.  W = M / 4 code words.
template <int W, int KPL>
__global__ __launch_bounds__(256) void scan_poly_kernel(ScanArgs a, PolyArgs pa, PolyLayout lay) {
    constexpr int M = 4 * W;
    const int MODE = a.table_mode;                     // (workgroup-uniform)
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    float* lut = reinterpret_cast<float*>(smraw);                                  // [M][ksub], later the merge area
    u64* selq = reinterpret_cast<u64*>(smraw + lay.selq);                          // [4][64]
    uint32_t* ring = reinterpret_cast<uint32_t*>(smraw + lay.ring);                // [4][kPolyRing]
    ProbeMeta pm;
    pm.carve(smraw + lay.meta, a.nprobe);
    unsigned long long* wg_pass = reinterpret_cast<unsigned long long*>(smraw + lay.misc);
    uint32_t* qcw = reinterpret_cast<uint32_t*>(smraw + lay.qcode);                // [W] the list's q_code
    uint8_t* qcb = reinterpret_cast<uint8_t*>(qcw);
    float* sres = reinterpret_cast<float*>(smraw + lay.sres);                      // [d] residual (MODE 0)

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t q = blockIdx.x;
    const int E = M * a.ksub;
    const int64_t* kq = a.keys + q * a.nprobe;
    const float* qt = a.qtab ? a.qtab + q * E : nullptr;
    const bool codes_only = pa.qcodes != nullptr;      // vlq_ivfpq_query_codes: the tables and q_code of every probe, no scan

    const bool badkey = probe_meta_fill(a, q, pm, t, 256);
    if (t == 0) *wg_pass = 0ull;
    __syncthreads();
    if (wave == 0) probe_meta_scan(a, pm, lane);       // prefix sums, the max_codes cut (IndexIVFPQ.cpp:1033)
    __syncthreads();

    // q_code[m] = first argmin_j lut[m][j]: (value, index) keys reduced across the lanes, the lower index wins.
    // + 0.0f folds -0 into +0, which the reference's `<` does not tell apart.
    auto argmin_codes = [&]() __attribute__((always_inline)) {
        for (int m = wave; m < M; m += 4) {
            u64 best = kMaxKey;
            for (int j = lane; j < a.ksub; j += 64) {
                const u64 key = ((u64)f32_to_ordered(__fadd_rn(lut[m * a.ksub + j], 0.0f)) << 32) | (uint32_t)j;
                best = umin64(best, key);
            }
#pragma unroll
            for (int stride = 32; stride > 0; stride >>= 1) best = umin64(best, shfl_xor_u64(best, stride));
            if (lane == 0) qcb[m] = (uint8_t)(uint32_t)best;
        }
    };
    if (MODE == 2) {
        // one distance table per query (IndexIVFPQ.cpp:558-559) and one code (:544-545)
        for (int e = t; e < E; e += 256) lut[e] = qt[e];
        __syncthreads();
        argmin_codes();
        __syncthreads();
    }

    WaveSelect<KPL> sel;
    sel.init(a.k, selq + wave * 64, lane);
    uint32_t* myring = ring + wave * kPolyRing;
    uint32_t npass = 0;                                // passers of this wave (wave-uniform)

    for (int p = 0; p < a.nprobe; p++) {
        int64_t key = pm.pkey[p];
        if (codes_only) { key = kq[p]; if (key >= a.nlist) key = -1; }
        if (key < 0) continue;                         // (workgroup-uniform)
        if (MODE != 2) {
            __syncthreads();                           // the previous list's table and q_code are no longer read
            if (MODE == 1) {
                if (a.imi_nbits > 0) {
                    // table type 2 (IndexIVFPQ.cpp:645-686): sub-quantizer m takes its row from the coarse sub-index of its half
                    const int64_t ki0 = key & ((int64_t(1) << a.imi_nbits) - 1), ki1 = key >> a.imi_nbits;
                    for (int e = t; e < E; e += 256) {
                        const int64_t ki = (e / a.ksub) < M / 2 ? ki0 : ki1;
                        lut[e] = __fadd_rn(a.term2[ki * E + e], __fmul_rn(-2.f, qt[e]));
                    }
                } else {
                    const float* t2 = a.term2 + key * E;         // fvec_madd, IndexIVFPQ.cpp:641-644
                    for (int e = t; e < E; e += 256) lut[e] = __fadd_rn(t2[e], __fmul_rn(-2.f, qt[e]));
                }
            } else {
                // compute_residual + compute_distance_table (IndexIVFPQ.cpp:636-637)
                const float* c = a.coarse + key * a.d;
                const float* qv = a.queries + q * a.d;
                for (int e = t; e < a.d; e += 256) sres[e] = __fsub_rn(qv[e], c[e]);
                __syncthreads();
                for (int e = t; e < E; e += 256) {
                    const float* xv = sres + (e / a.ksub) * a.dsub;
                    const float* cj = a.pq_cent + (size_t)e * a.dsub;
                    lut[e] = l2sqr_sse_order([&](int c2) { return xv[c2]; }, [&](int c2) { return cj[c2]; }, a.dsub);
                }
            }
            __syncthreads();
            argmin_codes();
            __syncthreads();
        }
        if (codes_only) {
            if (t < M) pa.qcodes[((size_t)q * a.nprobe + p) * M + t] = qcb[t];
            continue;
        }
        uint32_t qc[W];
#pragma unroll
        for (int i = 0; i < W; i++) qc[i] = __builtin_amdgcn_readfirstlane(qcw[i]);

        const uint32_t len = pm.plen[p], pos0 = pm.cum[p];
        const int64_t off = pm.poff[p];
        const float dis0 = MODE == 1 ? pm.pd0[p] : 0.f;         // IndexIVFPQ.cpp:638-639, :646
        // n passers waiting in the ring from slot h0 on: their codes again (cache hits), the look-ups left to right, the offer
        auto look_up = [&](uint32_t h0, uint32_t n) __attribute__((always_inline)) {
            const bool v = (uint32_t)lane < n;
            const uint32_t j = v ? myring[(h0 + lane) & (kPolyRing - 1)] : 0u;
            const PolyCode<W> c = poly_load<W>(a.codes, off + j);
            float dis = dis0;
            const float* tab = lut;
#pragma unroll
            for (int i = 0; i < W; i++) {
                const uint32_t cw = c.w[i];
                dis = __fadd_rn(dis, tab[cw & 255u]); tab += a.ksub;
                dis = __fadd_rn(dis, tab[(cw >> 8) & 255u]); tab += a.ksub;
                dis = __fadd_rn(dis, tab[(cw >> 16) & 255u]); tab += a.ksub;
                dis = __fadd_rn(dis, tab[cw >> 24]); tab += a.ksub;
            }
            sel.offer_keyed(dis, pos0 + j, v);
        };
        uint32_t head = 0, tail = 0;                   // (wave-uniform)
        for (uint32_t j0 = (uint32_t)wave * 64; j0 < len; j0 += 256) {
            const uint32_t j = j0 + lane;
            const PolyCode<W> c = poly_load<W>(a.codes, off + min(j, len - 1));
            int hd = 0;
#pragma unroll
            for (int i = 0; i < W; i++) hd += __popc(c.w[i] ^ qc[i]);
            const bool pass = j < len && hd < pa.ht;   // IndexIVFPQ.cpp:901
            const u64 mask = __ballot(pass);
            if (mask == 0) continue;
            if (pass) myring[(tail + __popcll(mask & ((1ull << lane) - 1ull))) & (kPolyRing - 1)] = j;
            tail += __popcll(mask);
            __builtin_amdgcn_wave_barrier();
            if (tail - head >= 64) { look_up(head, 64); head += 64; }
        }
        if (tail != head) look_up(head, tail - head);  // the table changes at the list boundary
        npass += tail;
        __builtin_amdgcn_wave_barrier();
    }
    if (codes_only) return;
    if (lane == 0 && npass) atomicAdd(wg_pass, (unsigned long long)npass);
    const unsigned long long nscan = pm.cum[a.nprobe];
    merge_and_emit<KPL>(sel, smraw, pm.cum, a, q, wave, lane,
                        [&](int p, int64_t& lkey, int64_t& loff) { lkey = kq[p]; loff = pm.poff[p]; });
    if (t == 0) {
        atomicAdd(a.ncode, nscan);
        atomicAdd(pa.n_pass, *wg_pass);                // indexIVFPQ_stats.n_hamming_pass (IndexIVFPQ.cpp:902, :1048)
    }
    if (badkey) *a.bad_key = 1;                        // (every thread looked at its own probes)
}

template <int W, int KPL>
static bool launch_poly_i(const ScanArgs& a, const PolyArgs& pa, const PolyLayout& lay, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(scan_poly_kernel<W, KPL>), lay.bytes);
    hipLaunchKernelGGL((scan_poly_kernel<W, KPL>), dim3((unsigned)a.nq), dim3(256), lay.bytes, s, a, pa, lay);
    return true;
}
template <int W>
static bool launch_poly_k(const ScanArgs& a, const PolyArgs& pa, const PolyLayout& lay, hipStream_t s) {
    if (a.table_mode < 0 || a.table_mode > 2) return false;
    if (a.k <= 64) return launch_poly_i<W, 1>(a, pa, lay, s);
    if (a.k <= 256) return launch_poly_i<W, 4>(a, pa, lay, s);
    return launch_poly_i<W, 16>(a, pa, lay, s);
}

bool launch_scan_poly(const ScanArgs& a, const PolyArgs& pa, hipStream_t s) {
    if (a.nq <= 0) return true;
    if (!poly_shape_ok(a.M, a.ksub) || a.nprobe > kPolyMaxProbes) return false;
    const PolyLayout lay = poly_layout(a.M, a.ksub, a.nprobe, a.k, a.d);
    switch (a.M / 4) {
#define VLQ_POLY(W) case W: return launch_poly_k<W>(a, pa, lay, s)
    VLQ_POLY(1); VLQ_POLY(2); VLQ_POLY(3); VLQ_POLY(4); VLQ_POLY(5); VLQ_POLY(6); VLQ_POLY(7); VLQ_POLY(8);
    VLQ_POLY(9); VLQ_POLY(10); VLQ_POLY(11); VLQ_POLY(12); VLQ_POLY(13); VLQ_POLY(14); VLQ_POLY(15); VLQ_POLY(16);
#undef VLQ_POLY
    }
    return false;
}

}  // namespace vlq
