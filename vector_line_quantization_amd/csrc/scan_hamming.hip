// faiss::IndexLSH on the device: the encoder (apply_preprocess + fvecs2bitvecs, IndexLSH.cpp:50-81, hamming.cpp:353-379) and the
// exhaustive Hamming scan (hammings_knn, hamming.cpp:264-341, :474-506).
//
// Scan: the grid is (query tile) x (code slice), decided by plan_hamming_scan (hamming_plan.h), as scan_pq.hip's:
//   * a workgroup of four waves keeps the codes of Q queries in LDS.  The query's words are wave-uniform: the first piece of
//     every query sits in scalar registers (a code of one piece -- 4, 8 or 16 bytes -- costs the loop no LDS access), further
//     pieces are read at one address by all lanes (a broadcast);
//   * it walks the codes of its slice once -- wave w takes rows lo + 64 w + 256 i + lane, a lane owns one stored code per trip and
//     loads it in pieces of 16, 8 or 4 bytes, the first piece of the next trip's code fetched while this trip's is counted -- and
//     XOR-popcounts every piece against the Q queries, accumulating through the popcount's add operand;
//   * the distance is an integer <= 1024, exact in f32; the key is (distance as ordered f32, position), the selection is
//     wave_topk.cuh's, unchanged.  A wave offers its candidates in increasing position, so the strict admission `dis < k-th`
//     decides by the full key: a code AT the current k-th distance -- with integer distances the common case -- is rejected by
//     one compare and one ballot, without entering the queue;
//   * at the slice end wave q joins the four waves' rows of query q and writes the final row (S == 1) or the slice's k keys to
//     scratch (S > 1: pq_join_kernel writes the rows).  The key order is total: the rows depend on neither Q nor S.
// Padding is (float)INT_MAX / -1 (Heap.h:76-78 through IndexLSH.cpp:154-155), not pq_emit's FLT_MAX: a row can hold padding
// only when k > ntotal, and then -- only then -- ham_pad_kernel rewrites the distance of every slot whose label is -1.
#include "scan_hamming.h"
#include "kernels.h"
#include "join_rows.cuh"
#include "wave_topk.cuh"

#include <type_traits>

namespace vlq {

namespace {

constexpr int kQWords = kHamMaxCode / 4;     // words of LDS per query code

template <int LOAD> struct HamPiece { typedef uint32_t type; };
template <> struct HamPiece<8> { typedef uint2 type; };
template <> struct HamPiece<16> { typedef uint4 type; };

template <int LOAD>
__device__ __forceinline__ int piece_hd(const typename HamPiece<LOAD>::type& v, const uint32_t* qw, int acc) {
    if constexpr (LOAD == 4) {
        return __builtin_popcount(v ^ qw[0]) + acc;
    } else {
        acc = __builtin_popcount(v.x ^ qw[0]) + acc;
        acc = __builtin_popcount(v.y ^ qw[1]) + acc;
        if constexpr (LOAD == 16) {
            acc = __builtin_popcount(v.z ^ qw[2]) + acc;
            acc = __builtin_popcount(v.w ^ qw[3]) + acc;
        }
        return acc;
    }
}

}  // namespace

template <int Q, int KPL, int LOAD>
__global__ __launch_bounds__(256) void scan_hamming_kernel(HamScanArgs a, HamLayout lay) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    u64* selq = reinterpret_cast<u64*>(smraw + lay.selq);                           // [4][Q][64]
    uint32_t* qcw = reinterpret_cast<uint32_t*>(smraw + lay.qcode);                 // [Q][kQWords]

    typedef typename HamPiece<LOAD>::type Piece;
    constexpr int NP = LOAD / 4;                       // words per piece

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t q0 = (int64_t)blockIdx.x * Q;
    const int slice = blockIdx.y;
    const int W = a.code_size >> 2;                    // code words (<= kQWords)
    const size_t cs = (size_t)a.code_size;

    if (t < Q * kQWords) {
        const int qi = t / kQWords, w = t % kQWords;
        qcw[t] = (q0 + qi < a.nq && w < W) ? reinterpret_cast<const uint32_t*>(a.qcodes)[(q0 + qi) * W + w] : 0u;
    }
    __syncthreads();

    WaveSelect<KPL> sel[Q];
#pragma unroll
    for (int qi = 0; qi < Q; qi++) sel[qi].init(a.k, selq + (size_t)(wave * Q + qi) * 64, lane);

    const int64_t lo = min((int64_t)slice * a.slice_len, a.ntotal), hi = min(lo + a.slice_len, a.ntotal);
    const uint8_t* __restrict__ codes = a.codes;

    uint32_t qfirst[Q][NP];
#pragma unroll
    for (int qi = 0; qi < Q; qi++) {
#pragma unroll
        for (int w = 0; w < NP; w++) qfirst[qi][w] = __builtin_amdgcn_readfirstlane(qcw[qi * kQWords + w]);
    }
    const int pieces = W / NP;
    Piece nxt = {};
    if (lo < hi) nxt = *reinterpret_cast<const Piece*>(codes + (size_t)min(lo + wave * 64 + lane, hi - 1) * cs);
    for (int64_t j0 = lo + wave * 64; j0 < hi; j0 += 256) {
        const int64_t j = j0 + lane;
        const bool valid = j < hi;
        const Piece* p = reinterpret_cast<const Piece*>(codes + (size_t)min(j, hi - 1) * cs);
        const Piece cur = nxt;
        nxt = *reinterpret_cast<const Piece*>(codes + (size_t)min(j + 256, hi - 1) * cs);       // the next trip's first piece
        int hd[Q];
#pragma unroll
        for (int qi = 0; qi < Q; qi++) hd[qi] = piece_hd<LOAD>(cur, qfirst[qi], 0);
        for (int c = 1; c < pieces; c++) {
            const Piece v = p[c];
#pragma unroll
            for (int qi = 0; qi < Q; qi++) hd[qi] = piece_hd<LOAD>(v, qcw + qi * kQWords + NP * c, hd[qi]);       // (one address: a broadcast)
        }
#pragma unroll
        for (int qi = 0; qi < Q; qi++) sel[qi].offer((float)hd[qi], (uint32_t)j, valid && q0 + qi < a.nq);
    }

    // wave q joins the four waves' rows of query q
#pragma unroll
    for (int qi = 0; qi < Q; qi++) sel[qi].flush();
    u64* mb = reinterpret_cast<u64*>(smraw);           // [Q][4][k]
    const int k = a.k;
#pragma unroll
    for (int qi = 0; qi < Q; qi++) {
#pragma unroll
        for (int r = 0; r < KPL; r++) {
            const int e = r * 64 + lane;
            if (e < k) mb[(size_t)(qi * kHamWaves + wave) * k + e] = sel[qi].best[r];
        }
    }
    __syncthreads();
#pragma unroll
    for (int qi = 0; qi < Q; qi++) {
        if (wave != qi || q0 + qi >= a.nq) continue;   // (wave-uniform)
        for (int w = 0; w < kHamWaves; w++) {
            if (w == wave) continue;
            for (int e0 = 0; e0 < k; e0 += 64) {
                const int e = e0 + lane;
                const bool valid = e < k;
                sel[qi].offer_key(valid ? mb[(size_t)(qi * kHamWaves + w) * k + e] : kMaxKey, valid);
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
            pq_emit<KPL>(sel[qi], k, 0u, a.D + q * k, a.I + q * k, lane);
        }
    }
}

// the padding of this index: a slot without a label carries (float)INT_MAX (IndexLSH.cpp:154-155 converts the heap's neutral
// element, Heap.h:76-78), where the shared emit wrote FLT_MAX
__global__ __launch_bounds__(256) void ham_pad_kernel(float* __restrict__ D, const int64_t* __restrict__ I, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n && I[e] < 0) D[e] = 2147483648.0f;
}

// One wave per (row, group of 64 bits); the four waves of a workgroup take consecutive items.
__global__ __launch_bounds__(256) void lsh_encode_kernel(const float* __restrict__ x, int64_t n, int d, int nbits, const float* __restrict__ At,
                                                         const float* __restrict__ b, const float* __restrict__ thr, float* __restrict__ xt_out,
                                                         uint8_t* __restrict__ codes_out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = (nbits + 63) >> 6, bpv = (nbits + 7) >> 3;
    const int64_t item = (int64_t)blockIdx.x * 4 + wave;
    if (item >= n * G) return;                         // (wave-uniform)
    const int64_t row = item / G;
    const int g = (int)(item % G);
    const int j = g * 64 + lane;
    const bool valid = j < nbits;
    const float* xr = x + (size_t)row * d;
    float xt = 0.f;
    if (valid) {
        if (At) {
            xt = b ? b[j] : 0.0f;
            for (int i = 0; i < d; i++) xt = fmaf(At[(size_t)i * nbits + j], xr[i], xt);
        } else {
            xt = xr[j];
        }
        if (thr) xt = __fsub_rn(xt, thr[j]);
        if (xt_out) xt_out[(size_t)row * nbits + j] = xt;
    }
    if (!codes_out) return;
    const u64 mask = __ballot(valid && xt >= 0.f);
    const int nbytes = min(8, bpv - g * 8);
    if (lane < nbytes) codes_out[(size_t)row * bpv + g * 8 + lane] = (uint8_t)(mask >> (8 * lane));
}

template <int Q, int KPL, int LOAD>
static void launch_ham_i(const HamScanArgs& a, const HamPlan& P, int64_t tiles, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(scan_hamming_kernel<Q, KPL, LOAD>), P.lay.bytes);
    hipLaunchKernelGGL((scan_hamming_kernel<Q, KPL, LOAD>), dim3((unsigned)tiles, (unsigned)P.S), dim3(256), P.lay.bytes, s, a, P.lay);
}
template <int Q, int KPL>
static bool launch_ham_load(const HamScanArgs& a, const HamPlan& P, int64_t tiles, hipStream_t s) {
    switch (P.load) {
        case 4: launch_ham_i<Q, KPL, 4>(a, P, tiles, s); return true;
        case 8: launch_ham_i<Q, KPL, 8>(a, P, tiles, s); return true;
        case 16: launch_ham_i<Q, KPL, 16>(a, P, tiles, s); return true;
    }
    return false;
}

bool launch_scan_hamming(const HamScanArgs& a, const HamPlan& P, hipStream_t s) {
    if (a.nq <= 0) return true;
    if (!P.ok || a.S != P.S || a.slice_len != P.slice_len || a.code_size % P.load != 0 || a.code_size > kHamMaxCode) return false;
    if (reinterpret_cast<uintptr_t>(a.codes) & (uintptr_t)(P.load - 1)) return false;
    if (reinterpret_cast<uintptr_t>(a.qcodes) & 3u) return false;
    const int64_t tiles = (a.nq + P.Q - 1) / P.Q;
    bool ok = false;
    if (P.kpl == 16) ok = P.Q == 1 && launch_ham_load<1, 16>(a, P, tiles, s);
    else if (P.kpl == 4) ok = P.Q == 1 ? launch_ham_load<1, 4>(a, P, tiles, s) : P.Q == 2 ? launch_ham_load<2, 4>(a, P, tiles, s) : P.Q == 4 && launch_ham_load<4, 4>(a, P, tiles, s);
    else if (P.kpl == 1) ok = P.Q == 1 ? launch_ham_load<1, 1>(a, P, tiles, s) : P.Q == 2 ? launch_ham_load<2, 1>(a, P, tiles, s) : P.Q == 4 && launch_ham_load<4, 1>(a, P, tiles, s);
    if (!ok) return false;
    if (P.join) launch_join_rows(P.kpl, a.part, a.nq, a.S, (int64_t)a.S * a.k, a.k, 0u, a.D, a.I, nullptr, 0, s);      // join_rows.cuh
    if (a.k > a.ntotal) {
        const int64_t e = a.nq * a.k;
        hipLaunchKernelGGL(ham_pad_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, a.D, a.I, e);
    }
    return true;
}

void launch_lsh_encode(const float* x, int64_t n, int d, int nbits, const float* At, const float* b, const float* thr, float* xt_out,
                       uint8_t* codes_out, hipStream_t s) {
    if (n <= 0) return;
    const int64_t items = n * ((nbits + 63) / 64);
    hipLaunchKernelGGL(lsh_encode_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, x, n, d, nbits, At, b, thr, xt_out, codes_out);
}

}  // namespace vlq
