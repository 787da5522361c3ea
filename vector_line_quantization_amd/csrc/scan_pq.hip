// Exhaustive PQ scan: faiss::IndexPQ::search (IndexPQ.cpp:124-203, :217-358) on the device.  Every query meets every code, so
// the grid is (query tile) x (code slice), decided by plan_pq_scan (pq_plan.h):
//   * a workgroup of four waves keeps the tables of Q queries in LDS, interleaved [m][j][Q]: one ds_read_b64 / ds_read_b128
//     returns the entries of 2 / 4 queries for one (m, byte), and one address computation serves Q look-ups;
//   * it walks the codes of its slice once -- wave w takes rows lo + 64 w + 256 i + lane, each byte of a code is loaded once --
//     and scores every code for the Q queries, one running selection (wave_topk.cuh) per (wave, query).  A wave offers its
//     candidates in increasing position, so the strict admission `dis < k-th` is the reference's heap rule (Heap.h:68-79);
//   * at the slice end wave q joins the four waves' rows of query q by the full (distance, position) key and writes the final
//     row (S == 1) or the slice's k keys to scratch (S > 1: pq_join_kernel writes the rows).  The key order is total: the rows
//     depend on neither Q nor S.
// Summation orders are template cases (pq_plan.h: PqOrder):
//   ST_PQ       pq_estimators_from_tables (ProductQuantizer.cpp:46-143): M == 4, M % 4 == 0 in groups of four, else from 0
//   ST_SDC      from 0, left to right (ProductQuantizer.cpp:643-648) over a per-query table gathered from sdc_table rows
//   polysemous  a code is looked up only if hd < ht (IndexPQ.cpp:237-247): hd = popcount of the XOR (FILTER 1) or the number of
//               differing bytes (FILTER 2, generalized_hamming_64, hamming.h:329-405).  Passers are compacted into a ring per
//               (wave, query); whenever 64 wait the wave looks a full row of them up, from 0, left to right.
// Inner product: the tables hold inner products, the sums are the reference's; the selection runs on the negated sum (negation
// is exact), the rows come out descending, padded -FLT_MAX.
#include "kernels.h"
#include "pq_plan.h"
#include "join_rows.cuh"
#include "wave_topk.cuh"

#include <type_traits>

namespace vlq {

template <int Q>
__device__ __forceinline__ void tab_read(const float* __restrict__ tab, uint32_t e, float (&t)[Q]) {
    if constexpr (Q == 1) {
        t[0] = tab[e];
    } else if constexpr (Q == 2) {
        const float2 v = reinterpret_cast<const float2*>(tab)[e];
        t[0] = v.x; t[1] = v.y;
    } else {
        const float4 v = reinterpret_cast<const float4*>(tab)[e];
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
    }
}

// four sub-quantizers of one code word for the Q queries of the tile; base = m * ksub on entry, (m + 4) * ksub on return
template <int Q, int ORDER>
__device__ __forceinline__ void score_word(const float* __restrict__ tab, uint32_t cw, uint32_t ksub, uint32_t& base, float (&dis)[Q]) {
    float t0[Q], t1[Q], t2[Q], t3[Q];
    tab_read<Q>(tab, base + (cw & 255u), t0); base += ksub;
    tab_read<Q>(tab, base + ((cw >> 8) & 255u), t1); base += ksub;
    tab_read<Q>(tab, base + ((cw >> 16) & 255u), t2); base += ksub;
    tab_read<Q>(tab, base + (cw >> 24), t3); base += ksub;
#pragma unroll
    for (int q = 0; q < Q; q++) {
        if constexpr (ORDER == kPqOrderLeft) {
            dis[q] = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(dis[q], t0[q]), t1[q]), t2[q]), t3[q]);
        } else {
            const float dism = __fadd_rn(__fadd_rn(__fadd_rn(t0[q], t1[q]), t2[q]), t3[q]);
            dis[q] = ORDER == kPqOrderM4 ? dism : __fadd_rn(dis[q], dism);
        }
    }
}

template <int FILTER>
__device__ __forceinline__ int code_hd(uint32_t x) {
    if constexpr (FILTER == 1) return __popc(x);
    // differing bytes (generalized_hamming_64): OR every byte's bits into its lowest one
    x |= x >> 1; x |= x >> 2; x |= x >> 4;
    return __popc(x & 0x01010101u);
}

// LOAD: bytes of a code per global load (16: rows of M % 16 == 0 bytes, 4: M % 4 == 0, 1: any M)
template <int Q, int KPL, int ORDER, int FILTER, int LOAD>
__global__ __launch_bounds__(256) void scan_pq_kernel(PqScanArgs a, PqLayout lay) {
    static_assert(LOAD != 1 || (ORDER == kPqOrderLeft && FILTER == 0), "byte loads serve the plain left-to-right order only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    float* tab = reinterpret_cast<float*>(smraw);                                   // [M][ksub][Q], later the merge area
    u64* selq = reinterpret_cast<u64*>(smraw + lay.selq);                           // [4][Q][64]
    uint32_t* ring = reinterpret_cast<uint32_t*>(smraw + lay.ring);                 // [4][Q][kPqRing]
    uint32_t* qcw = reinterpret_cast<uint32_t*>(smraw + lay.qcode);                 // [Q][16]
    unsigned long long* wg_pass = reinterpret_cast<unsigned long long*>(smraw + lay.misc);

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t q0 = (int64_t)blockIdx.x * Q;
    const int slice = blockIdx.y;
    const int E = a.M * a.ksub;
    const int W = a.M >> 2;                            // code words (LOAD != 1)
    const uint32_t ksub = (uint32_t)a.ksub;

    for (int e = t; e < E; e += 256) {
#pragma unroll
        for (int qi = 0; qi < Q; qi++) tab[(size_t)e * Q + qi] = q0 + qi < a.nq ? a.qtab[(q0 + qi) * E + e] : 0.f;
    }
    if constexpr (FILTER != 0) {
        if (t < Q * 16) {
            const int qi = t >> 4, w = t & 15;
            qcw[t] = (q0 + qi < a.nq && w < W) ? reinterpret_cast<const uint32_t*>(a.qcodes)[(q0 + qi) * W + w] : 0u;
        }
        if (t == 0) *wg_pass = 0ull;
    }
    __syncthreads();

    WaveSelect<KPL> sel[Q];
#pragma unroll
    for (int qi = 0; qi < Q; qi++) sel[qi].init(a.k, selq + (size_t)(wave * Q + qi) * 64, lane);

    const int64_t lo = min((int64_t)slice * a.slice_len, a.ntotal), hi = min(lo + a.slice_len, a.ntotal);
    const uint8_t* __restrict__ codes = a.codes;
    const size_t M = (size_t)a.M;

    if constexpr (FILTER == 0) {
        uint4 nxt = make_uint4(0, 0, 0, 0);
        if constexpr (LOAD == 16) {
            const int64_t j = lo + wave * 64 + lane;
            if (lo < hi) nxt = *reinterpret_cast<const uint4*>(codes + (size_t)min(j, hi - 1) * M);
        }
        for (int64_t j0 = lo + wave * 64; j0 < hi; j0 += 256) {
            const int64_t j = j0 + lane;
            const bool valid = j < hi;
            const uint8_t* row = codes + (size_t)min(j, hi - 1) * M;
            float dis[Q];
#pragma unroll
            for (int qi = 0; qi < Q; qi++) dis[qi] = 0.f;
            uint32_t base = 0;
            if constexpr (LOAD == 16) {
                const uint4 cur = nxt;
                nxt = *reinterpret_cast<const uint4*>(codes + (size_t)min(j + 256, hi - 1) * M);   // the next trip's first piece
                const uint4* p = reinterpret_cast<const uint4*>(row);
                for (int c = 0; c < (W >> 2); c++) {
                    const uint4 v = c == 0 ? cur : p[c];
                    score_word<Q, ORDER>(tab, v.x, ksub, base, dis);
                    score_word<Q, ORDER>(tab, v.y, ksub, base, dis);
                    score_word<Q, ORDER>(tab, v.z, ksub, base, dis);
                    score_word<Q, ORDER>(tab, v.w, ksub, base, dis);
                }
            } else if constexpr (LOAD == 4) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(row);
                for (int c = 0; c < W; c++) score_word<Q, ORDER>(tab, p[c], ksub, base, dis);
            } else {
                for (int m = 0; m < a.M; m++) {
                    float tq[Q];
                    tab_read<Q>(tab, base + row[m], tq);
                    base += ksub;
#pragma unroll
                    for (int qi = 0; qi < Q; qi++) dis[qi] = __fadd_rn(dis[qi], tq[qi]);
                }
            }
#pragma unroll
            for (int qi = 0; qi < Q; qi++) sel[qi].offer(flip_sign(dis[qi], a.neg), (uint32_t)j, valid && q0 + qi < a.nq);
        }
    } else {
        uint32_t head[Q], tail[Q];                     // (wave-uniform) ring cursors; tail = passers so far
#pragma unroll
        for (int qi = 0; qi < Q; qi++) head[qi] = tail[qi] = 0u;
        // n passers of query qi waiting from slot h0 on: their codes again (cache hits), from 0, left to right (IndexPQ.cpp:242-247)
        auto look_up = [&](auto qc, uint32_t h0, uint32_t n) __attribute__((always_inline)) {
            constexpr int qi = decltype(qc)::value;
            const uint32_t* myring = ring + (size_t)(wave * Q + qi) * kPqRing;
            const bool v = (uint32_t)lane < n;
            const int64_t j = lo + (v ? myring[(h0 + lane) & (kPqRing - 1)] : 0u);
            const uint32_t* p = reinterpret_cast<const uint32_t*>(codes + (size_t)j * M);
            float dis = 0.f;
            const float* tq = tab + qi;
            uint32_t base = 0;
            for (int c = 0; c < W; c++) {
                const uint32_t cw = p[c];
                dis = __fadd_rn(dis, tq[(size_t)(base + (cw & 255u)) * Q]); base += ksub;
                dis = __fadd_rn(dis, tq[(size_t)(base + ((cw >> 8) & 255u)) * Q]); base += ksub;
                dis = __fadd_rn(dis, tq[(size_t)(base + ((cw >> 16) & 255u)) * Q]); base += ksub;
                dis = __fadd_rn(dis, tq[(size_t)(base + (cw >> 24)) * Q]); base += ksub;
            }
            sel[qi].offer(dis, (uint32_t)j, v);
        };
        auto each_query = [&](auto f) __attribute__((always_inline)) {
            f(std::integral_constant<int, 0>());
            if constexpr (Q > 1) f(std::integral_constant<int, 1>());
            if constexpr (Q > 2) { f(std::integral_constant<int, 2>()); f(std::integral_constant<int, 3>()); }
        };
        // a code is read in pieces of 16 bytes (LOAD 16) or 8 (code_size % 8 == 0).  The first piece of the next trip's code is
        // fetched while this trip's is counted, and the queries' first pieces stay in scalar registers: a code of one piece
        // (M = 16, M = 8) costs the loop no LDS access at all
        constexpr int NP = LOAD == 16 ? 4 : 2;         // words per piece
        typedef typename std::conditional<LOAD == 16, uint4, uint2>::type Piece;
        auto piece_hd = [&](const Piece& v, const uint32_t* qw) __attribute__((always_inline)) {
            int h = code_hd<FILTER>(v.x ^ qw[0]) + code_hd<FILTER>(v.y ^ qw[1]);
            if constexpr (LOAD == 16) h += code_hd<FILTER>(v.z ^ qw[2]) + code_hd<FILTER>(v.w ^ qw[3]);
            return h;
        };
        uint32_t qfirst[Q][NP];
#pragma unroll
        for (int qi = 0; qi < Q; qi++) {
#pragma unroll
            for (int w = 0; w < NP; w++) qfirst[qi][w] = __builtin_amdgcn_readfirstlane(qcw[qi * 16 + w]);
        }
        const int pieces = W / NP;
        Piece nxt = {};
        if (lo < hi) nxt = *reinterpret_cast<const Piece*>(codes + (size_t)min(lo + wave * 64 + lane, hi - 1) * M);
        for (int64_t j0 = lo + wave * 64; j0 < hi; j0 += 256) {
            const int64_t j = j0 + lane;
            const bool valid = j < hi;
            const Piece* p = reinterpret_cast<const Piece*>(codes + (size_t)min(j, hi - 1) * M);
            const Piece cur = nxt;
            nxt = *reinterpret_cast<const Piece*>(codes + (size_t)min(j + 256, hi - 1) * M);
            int hd[Q];
#pragma unroll
            for (int qi = 0; qi < Q; qi++) hd[qi] = piece_hd(cur, qfirst[qi]);
            for (int c = 1; c < pieces; c++) {
                const Piece v = p[c];
#pragma unroll
                for (int qi = 0; qi < Q; qi++) hd[qi] += piece_hd(v, qcw + qi * 16 + NP * c);       // (one address: a broadcast)
            }
            each_query([&](auto qc) __attribute__((always_inline)) {
                constexpr int qi = decltype(qc)::value;
                const bool pass = valid && q0 + qi < a.nq && hd[qi] < a.ht;        // IndexPQ.cpp:239
                const u64 mask = __ballot(pass);
                if (mask == 0) return;
                uint32_t* myring = ring + (size_t)(wave * Q + qi) * kPqRing;
                if (pass) myring[(tail[qi] + __popcll(mask & ((1ull << lane) - 1ull))) & (kPqRing - 1)] = (uint32_t)(j - lo);
                tail[qi] += __popcll(mask);
                __builtin_amdgcn_wave_barrier();
                if (tail[qi] - head[qi] >= 64) { look_up(qc, head[qi], 64); head[qi] += 64; }
            });
        }
        uint32_t npass = 0;
        each_query([&](auto qc) __attribute__((always_inline)) {
            constexpr int qi = decltype(qc)::value;
            if (tail[qi] != head[qi]) look_up(qc, head[qi], tail[qi] - head[qi]);
            npass += tail[qi];
        });
        if (lane == 0 && npass) atomicAdd(wg_pass, (unsigned long long)npass);
    }

    // wave q joins the four waves' rows of query q
#pragma unroll
    for (int qi = 0; qi < Q; qi++) sel[qi].flush();
    __syncthreads();                                   // the tables are no longer read
    u64* mb = reinterpret_cast<u64*>(smraw);           // [Q][4][k]
    const int k = a.k;
#pragma unroll
    for (int qi = 0; qi < Q; qi++) {
#pragma unroll
        for (int r = 0; r < KPL; r++) {
            const int e = r * 64 + lane;
            if (e < k) mb[(size_t)(qi * kPqWaves + wave) * k + e] = sel[qi].best[r];
        }
    }
    __syncthreads();
    if constexpr (FILTER != 0) {
        if (t == 0 && *wg_pass) atomicAdd(a.n_pass, *wg_pass);          // indexPQ_stats.n_hamming_pass (IndexPQ.cpp:355)
    }
#pragma unroll
    for (int qi = 0; qi < Q; qi++) {
        if (wave != qi || q0 + qi >= a.nq) continue;   // (wave-uniform)
        for (int w = 0; w < kPqWaves; w++) {
            if (w == wave) continue;
            for (int e0 = 0; e0 < k; e0 += 64) {
                const int e = e0 + lane;
                const bool valid = e < k;
                sel[qi].offer_key(valid ? mb[(size_t)(qi * kPqWaves + w) * k + e] : kMaxKey, valid);
            }
        }
        sel[qi].flush();
        const int64_t q = q0 + qi;
        if (a.S > 1) {
            u64* out = a.part + ((size_t)q * a.S + slice) * k;
#pragma unroll
            for (int r = 0; r < KPL; r++) {
                const int e = r * 64 + lane;
                if (e < k) out[e] = sel[qi].best[r];
            }
        } else {
            pq_emit<KPL>(sel[qi], k, a.neg, a.D + q * k, a.I + q * k, lane);
        }
    }
}

// compute_code_from_distance_table (ProductQuantizer.cpp:363-383): the first j with tab[m][j] below everything before it, from
// 1e20; no such j leaves idxm = -1, stored as 255.  One wave per (vector, m).
__global__ __launch_bounds__(256) void pq_table_argmin_kernel(const float* __restrict__ tabs, int64_t n, int M, int ksub, uint8_t* __restrict__ codes) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= n * M) return;
    const float* row = tabs + (size_t)item * ksub;
    u64 best = kMaxKey;
    for (int j = lane; j < ksub; j += 64) {
        const float v = row[j];
        if (v < 1e20f) best = umin64(best, ((u64)f32_to_ordered(__fadd_rn(v, 0.0f)) << 32) | (uint32_t)j);     // (-0 is not below +0)
    }
#pragma unroll
    for (int stride = 32; stride > 0; stride >>= 1) best = umin64(best, shfl_xor_u64(best, stride));
    if (lane == 0) codes[item] = best == kMaxKey ? (uint8_t)255 : (uint8_t)(uint32_t)best;
}

// compute_sdc_table (ProductQuantizer.cpp:595-616): sdc[m][i + j * ksub] = sum_c (ci[c] - cj[c])^2, a scalar left-to-right sum
__global__ __launch_bounds__(256) void pq_sdc_table_kernel(const float* __restrict__ cent, int M, int ksub, int dsub, float* __restrict__ sdc) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)M * ksub * ksub) return;
    const int i = (int)(e % ksub), j = (int)((e / ksub) % ksub), m = (int)(e / ((int64_t)ksub * ksub));
    const float* ci = cent + ((size_t)m * ksub + i) * dsub;
    const float* cj = cent + ((size_t)m * ksub + j) * dsub;
    float accu = 0.f;
    for (int c = 0; c < dsub; c++) {
        const float df = __fsub_rn(ci[c], cj[c]);
        accu = __fadd_rn(accu, __fmul_rn(df, df));
    }
    sdc[e] = accu;
}

// the table search_sdc reads for query q (ProductQuantizer.cpp:644-648): tab[q][m][b] = sdc[m][b + qcode[q][m] * ksub]
__global__ __launch_bounds__(256) void pq_sdc_gather_kernel(const float* __restrict__ sdc, const uint8_t* __restrict__ qcodes, int64_t n, int M,
                                                            int ksub, float* __restrict__ tabs) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * M * ksub) return;
    const int b = (int)(e % ksub);
    const int64_t qm = e / ksub;
    const int m = (int)(qm % M);
    // (a query code of 255 with ksub < 256 -- no centroid below 1e20 -- reads row ksub - 1: the reference reads past its table there)
    const int qc = min((int)qcodes[qm], ksub - 1);
    tabs[e] = sdc[((size_t)m * ksub + qc) * ksub + b];
}

__global__ __launch_bounds__(256) void pq_iota_kernel(int64_t* __restrict__ out, int64_t n, int64_t base) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = base + i;
}

template <int Q, int KPL, int ORDER, int FILTER, int LOAD>
static void launch_pq_i(const PqScanArgs& a, const PqPlan& P, int64_t tiles, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(scan_pq_kernel<Q, KPL, ORDER, FILTER, LOAD>), P.lay.bytes);
    hipLaunchKernelGGL((scan_pq_kernel<Q, KPL, ORDER, FILTER, LOAD>), dim3((unsigned)tiles, (unsigned)P.S), dim3(256), P.lay.bytes, s, a, P.lay);
}
template <int Q, int KPL>
static bool launch_pq_mode(const PqScanArgs& a, const PqPlan& P, int64_t tiles, hipStream_t s) {
    const int mode = P.order * 100 + P.filter * 20 + P.load;
    switch (mode) {
        case kPqOrderM4 * 100 + 4: launch_pq_i<Q, KPL, kPqOrderM4, 0, 4>(a, P, tiles, s); return true;
        case kPqOrderGroup4 * 100 + 4: launch_pq_i<Q, KPL, kPqOrderGroup4, 0, 4>(a, P, tiles, s); return true;
        case kPqOrderGroup4 * 100 + 16: launch_pq_i<Q, KPL, kPqOrderGroup4, 0, 16>(a, P, tiles, s); return true;
        case kPqOrderLeft * 100 + 4: launch_pq_i<Q, KPL, kPqOrderLeft, 0, 4>(a, P, tiles, s); return true;
        case kPqOrderLeft * 100 + 1: launch_pq_i<Q, KPL, kPqOrderLeft, 0, 1>(a, P, tiles, s); return true;
        case kPqOrderLeft * 100 + 20 + 4: launch_pq_i<Q, KPL, kPqOrderLeft, 1, 4>(a, P, tiles, s); return true;
        case kPqOrderLeft * 100 + 20 + 16: launch_pq_i<Q, KPL, kPqOrderLeft, 1, 16>(a, P, tiles, s); return true;
        case kPqOrderLeft * 100 + 40 + 4: launch_pq_i<Q, KPL, kPqOrderLeft, 2, 4>(a, P, tiles, s); return true;
    }
    return false;
}

bool launch_scan_pq(const PqScanArgs& a, const PqPlan& P, hipStream_t s) {
    if (a.nq <= 0) return true;
    if (!P.ok || a.S != P.S || a.slice_len != P.slice_len) return false;
    if (P.load == 16 && (reinterpret_cast<uintptr_t>(a.codes) & 15u)) return false;
    if (P.load != 1 && (reinterpret_cast<uintptr_t>(a.codes) & 7u)) return false;
    const int64_t tiles = (a.nq + P.Q - 1) / P.Q;
    bool ok = false;
    if (P.kpl == 16) ok = P.Q == 1 && launch_pq_mode<1, 16>(a, P, tiles, s);
    else if (P.kpl == 4) ok = P.Q == 1 ? launch_pq_mode<1, 4>(a, P, tiles, s) : P.Q == 2 ? launch_pq_mode<2, 4>(a, P, tiles, s) : launch_pq_mode<4, 4>(a, P, tiles, s);
    else ok = P.Q == 1 ? launch_pq_mode<1, 1>(a, P, tiles, s) : P.Q == 2 ? launch_pq_mode<2, 1>(a, P, tiles, s) : launch_pq_mode<4, 1>(a, P, tiles, s);
    if (!ok) return false;
    if (P.join) launch_join_rows(P.kpl, a.part, a.nq, a.S, (int64_t)a.S * a.k, a.k, a.neg, a.D, a.I, nullptr, 0, s);      // join_rows.cuh
    return true;
}

void launch_pq_table_argmin(const float* tabs, int64_t n, int M, int ksub, uint8_t* codes, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pq_table_argmin_kernel, dim3((unsigned)((n * M + 3) / 4)), dim3(256), 0, s, tabs, n, M, ksub, codes);
}
void launch_pq_sdc_table(const float* cent, int M, int ksub, int dsub, float* sdc, hipStream_t s) {
    const int64_t n = (int64_t)M * ksub * ksub;
    hipLaunchKernelGGL(pq_sdc_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cent, M, ksub, dsub, sdc);
}
void launch_pq_sdc_gather(const float* sdc, const uint8_t* qcodes, int64_t n, int M, int ksub, float* tabs, hipStream_t s) {
    if (n <= 0) return;
    const int64_t e = n * M * ksub;
    hipLaunchKernelGGL(pq_sdc_gather_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, sdc, qcodes, n, M, ksub, tabs);
}
void launch_iota(int64_t* out, int64_t n, int64_t base, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pq_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, base);
}

}  // namespace vlq
