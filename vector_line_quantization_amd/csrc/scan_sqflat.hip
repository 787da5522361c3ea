// Exhaustive scalar-quantizer scan: faiss::IndexScalarQuantizer::search (IndexScalarQuantizer.cpp:727-781) on the device, with
// the encoder of its add (:719-725, encode_vector :446-455, :520-529) and the decoder of its reconstruct_n (:789-797).
// Every query meets every code, so the grid is (query tile) x (code slice), decided by plan_sqflat_scan (sqflat_plan.h):
//   * a workgroup of four waves keeps the Q queries of its tile in LDS, interleaved [i][Q]: one broadcast ds_read_b128 /
//     ds_read_b64 returns component i of 4 / 2 queries;
//   * it walks the codes of its slice once -- wave w takes rows w*64 .. w*64+63 of every 256, one lane owns one stored code --
//     decodes every component ONCE (sq_decode of sq_codec.cuh) and applies sq_accumulate for each query of the tile: Q x 8
//     accumulators under ORDER8 (component i into accumulator i % 8, joined by sq_join8(acc, 0.f)), Q accumulators from 0.f
//     otherwise.  The float operations are those stated in the header comment of scan_sq.hip, with three differences from the
//     IVF index: y is the query itself (no residual), accu0 is the constant 0 -- under inner product and ORDER8 the result is
//     still (0.f + lo) + hi, an addition that -0.f makes observable -- and there is no probe walk;
//   * every (wave, query) has a running selection (wave_topk.cuh) offered with offer_keyed(IP ? -v : v, position): FLT_MAX is
//     never admitted and an equal value never replaces an earlier one, which is `accu < simi[0]` / `accu > simi[0]` in scan
//     order (:751, :771);
//   * at the slice end wave q joins the four waves' rows of query q by the full (distance, position) key and writes the final
//     row (S == 1, pq_emit) or the slice's k keys to scratch (S > 1: pq_join_kernel of join_rows.cuh writes the rows).  The key
//     order is total: the rows depend on neither Q nor S.  No atomics.
// The reference never reorders its heap here (maxheap_reorder / minheap_reorder are called in search_with_probes_*, :917,
// :955, but not in IndexScalarQuantizer::search), so its rows come back in heap order.  The device returns them sorted by the
// library's total order -- distance ascending (inner product: descending), then position ascending -- padded FLT_MAX / -1
// (inner product: -FLT_MAX / -1).  Parity with the reference is therefore stated on sorted rows.
// Tail queries of the last tile run on the tile's first query and are masked at the offer.
// Read paths are sq_plan.h's: kSqReadTile128 turns 64 x 128 B tiles through the wave's own LDS area, kSqReadLane lets every
// lane walk its own row.  Plain VALU f32 with explicit __f*_rn throughout: an MFMA is an fmaf chain and would differ in bits.
#include "kernels.h"
#include "sqflat_plan.h"
#include "sq_codec.cuh"
#include "join_rows.cuh"
#include "wave_topk.cuh"

namespace vlq {

namespace {

// component i of the tile's Q queries: one address for the whole wave (a broadcast read)
template <int Q>
__device__ __forceinline__ void sqf_query_read(const float* __restrict__ sy, int i, float (&y)[Q]) {
    if constexpr (Q == 1) {
        y[0] = sy[i];
    } else if constexpr (Q == 2) {
        const float2 v = reinterpret_cast<const float2*>(sy)[i];
        y[0] = v.x; y[1] = v.y;
    } else {
        const v4f v = reinterpret_cast<const v4f*>(sy)[i];
        y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
    }
}

// components i0 .. i0+7 (i0 % 8 == 0) of one code, decoded once, into the eight accumulators of every query.  8 bits: the
// bytes of w0, w1; 4 bits: the nibbles of w0, low nibble first (component i in byte i / 2, :92, :98-105).
template <int Q, bool IP, int BITS, bool UNIFORM>
__device__ __forceinline__ void sqf_group8(uint32_t w0, uint32_t w1, const float* __restrict__ sy, const SqRange& R, int i0, float (&a)[Q][8]) {
    v4f m0, m1, f0, f1;
    if constexpr (UNIFORM) {
        m0 = m1 = v4f{R.vmin0, R.vmin0, R.vmin0, R.vmin0};
        f0 = f1 = v4f{R.vdiff0, R.vdiff0, R.vdiff0, R.vdiff0};
    } else {
        m0 = *reinterpret_cast<const v4f*>(R.vmin + i0); m1 = *reinterpret_cast<const v4f*>(R.vmin + i0 + 4);
        f0 = *reinterpret_cast<const v4f*>(R.vdiff + i0); f1 = *reinterpret_cast<const v4f*>(R.vdiff + i0 + 4);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t c;
        if constexpr (BITS == 8) c = ((j < 4 ? w0 : w1) >> (8 * (j & 3))) & 0xffu;
        else c = (w0 >> (4 * j)) & 0xfu;
        const float vm = j < 4 ? m0[j & 3] : m1[j & 3];
        const float vd = j < 4 ? f0[j & 3] : f1[j & 3];
        const float rec = sq_decode<BITS, true>(c, vm, vd);
        float y[Q];
        sqf_query_read<Q>(sy, i0 + j, y);
#pragma unroll
        for (int qi = 0; qi < Q; qi++) a[qi][j] = sq_accumulate<IP>(a[qi][j], y[qi], rec);
    }
}

// 16 bytes of one code, components i0 .. (16 at 8 bits, 32 at 4 bits)
template <int Q, bool IP, int BITS, bool UNIFORM>
__device__ __forceinline__ void sqf_unit16(const v4u u, const float* __restrict__ sy, const SqRange& R, int i0, float (&a)[Q][8]) {
    if constexpr (BITS == 8) {
        sqf_group8<Q, IP, 8, UNIFORM>(u.x, u.y, sy, R, i0, a);
        sqf_group8<Q, IP, 8, UNIFORM>(u.z, u.w, sy, R, i0 + 8, a);
    } else {
        sqf_group8<Q, IP, 4, UNIFORM>(u.x, 0u, sy, R, i0, a);
        sqf_group8<Q, IP, 4, UNIFORM>(u.y, 0u, sy, R, i0 + 8, a);
        sqf_group8<Q, IP, 4, UNIFORM>(u.z, 0u, sy, R, i0 + 16, a);
        sqf_group8<Q, IP, 4, UNIFORM>(u.w, 0u, sy, R, i0 + 24, a);
    }
}

}  // namespace

template <int Q, int KPL, bool IP, int BITS, bool UNIFORM, bool ORDER8>
__global__ __launch_bounds__(256) void scan_sqflat_kernel(SqFlatScanArgs a, SqFlatLayout lay, int code_size, int tile_read) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    u64* selq = reinterpret_cast<u64*>(smraw + lay.selq);                          // [4][Q][64]
    float* sy = reinterpret_cast<float*>(smraw + lay.sq);                          // [d][Q] the tile's queries
    float* svmin = reinterpret_cast<float*>(smraw + lay.vmin);                     // [d]
    float* svdiff = reinterpret_cast<float*>(smraw + lay.vdiff);                   // [d]

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t q0 = (int64_t)blockIdx.x * Q;
    const int slice = blockIdx.y;
    const int d = a.d;
    unsigned char* tile = smraw + wave * 64 * kSqTileStride;                       // this wave's [64][kSqTileStride]

    SqRange R;
    R.vmin = svmin; R.vdiff = svdiff;
    R.vmin0 = UNIFORM ? a.trained[0] : 0.f;
    R.vdiff0 = UNIFORM ? a.trained[1] : 0.f;
    for (int e = t; e < d * Q; e += 256) {
        const int i = e / Q, qi = e % Q;
        const int64_t q = q0 + qi < a.nq ? q0 + qi : q0;       // a tail query runs on the tile's first one
        sy[e] = a.queries[q * d + i];
    }
    if constexpr (!UNIFORM) {
        for (int e = t; e < d; e += 256) { svmin[e] = a.trained[e]; svdiff[e] = a.trained[d + e]; }
    }
    __syncthreads();

    WaveSelect<KPL> sel[Q];
#pragma unroll
    for (int qi = 0; qi < Q; qi++) sel[qi].init(a.k, selq + (size_t)(wave * Q + qi) * 64, lane);
    bool live[Q];
#pragma unroll
    for (int qi = 0; qi < Q; qi++) live[qi] = q0 + qi < a.nq;

    // the slice: rows lo .. hi-1 of the codes; j counts from lo (len < 2^32), the offered position is lo + j
    const int64_t lo = min((int64_t)slice * a.slice_len, a.ntotal), hi = min(lo + a.slice_len, a.ntotal);
    const uint32_t len = (uint32_t)(hi - lo), pos0 = (uint32_t)lo;
    const uint8_t* base = a.codes + (size_t)lo * code_size;
    uint32_t j0 = (uint32_t)wave * 64;

    if (j0 < len) {
        if constexpr (ORDER8) {
            if (tile_read) {
                constexpr int kCompPerUnit = BITS == 8 ? 16 : 32;        // components in 16 bytes of a code
                SqTile cur = sq_tile_load(base, j0, 0, len, code_size, lane);
                for (; j0 < len; j0 += 256) {
                    float acc[Q][8];
#pragma unroll
                    for (int qi = 0; qi < Q; qi++)
#pragma unroll
                        for (int r = 0; r < 8; r++) acc[qi][r] = 0.f;
                    for (int c0 = 0; c0 < code_size; c0 += kSqChunk) {
                        // the next tile is on its way while this one is turned and consumed
                        const bool last = c0 + kSqChunk >= code_size;
                        const SqTile nxt = sq_tile_load(base, last ? j0 + 256 : j0, last ? 0 : c0 + kSqChunk, len, code_size, lane);
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            *reinterpret_cast<v4u*>(tile + (i * 8 + (lane >> 3)) * kSqTileStride + (lane & 7) * 16) = cur.r[i];
                        __builtin_amdgcn_wave_barrier();   // (the wave's own area: its LDS accesses complete in order)
                        const unsigned char* row = tile + lane * kSqTileStride;
                        const int nunit = min(kSqChunk, code_size - c0) >> 4;
                        const int i0 = (c0 >> 4) * kCompPerUnit;
#pragma unroll
                        for (int c = 0; c < 8; c++) {
                            if (c < nunit) {
                                const v4u u = *reinterpret_cast<const v4u*>(row + 16 * c);
                                sqf_unit16<Q, IP, BITS, UNIFORM>(u, sy, R, i0 + c * kCompPerUnit, acc);
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
                        cur = nxt;
                    }
                    const uint32_t j = j0 + lane;
#pragma unroll
                    for (int qi = 0; qi < Q; qi++) {
                        const float v = sq_join8<IP>(acc[qi], 0.f);
                        sel[qi].offer_keyed(IP ? -v : v, pos0 + j, j < len && live[qi]);
                    }
                }
            } else {
                for (; j0 < len; j0 += 256) {
                    const uint32_t j = j0 + lane;
                    const uint8_t* row = base + (size_t)min(j, len - 1) * code_size;
                    float acc[Q][8];
#pragma unroll
                    for (int qi = 0; qi < Q; qi++)
#pragma unroll
                        for (int r = 0; r < 8; r++) acc[qi][r] = 0.f;
                    for (int i0 = 0; i0 < d; i0 += 8) {
                        if constexpr (BITS == 8) {       // rows of d bytes, d % 8 == 0: 8-byte aligned
                            const uint2 w = *reinterpret_cast<const uint2*>(row + i0);
                            sqf_group8<Q, IP, 8, UNIFORM>(w.x, w.y, sy, R, i0, acc);
                        } else {                         // rows of d / 2 bytes: 4-byte aligned
                            const uint32_t w = *reinterpret_cast<const uint32_t*>(row + (i0 >> 1));
                            sqf_group8<Q, IP, 4, UNIFORM>(w, 0u, sy, R, i0, acc);
                        }
                    }
#pragma unroll
                    for (int qi = 0; qi < Q; qi++) {
                        const float v = sq_join8<IP>(acc[qi], 0.f);
                        sel[qi].offer_keyed(IP ? -v : v, pos0 + j, j < len && live[qi]);
                    }
                }
            }
        } else {
            for (; j0 < len; j0 += 256) {
                const uint32_t j = j0 + lane;
                const uint8_t* row = base + (size_t)min(j, len - 1) * code_size;
                float acc[Q];
#pragma unroll
                for (int qi = 0; qi < Q; qi++) acc[qi] = 0.f;
                for (int i = 0; i < d; i++) {
                    uint32_t c;
                    if constexpr (BITS == 8) c = row[i];
                    else c = (row[i >> 1] >> ((i & 1) << 2)) & 0xfu;
                    const float vm = UNIFORM ? R.vmin0 : svmin[i], vd = UNIFORM ? R.vdiff0 : svdiff[i];
                    const float rec = sq_decode<BITS, false>(c, vm, vd);
                    float y[Q];
                    sqf_query_read<Q>(sy, i, y);
#pragma unroll
                    for (int qi = 0; qi < Q; qi++) acc[qi] = sq_accumulate<IP>(acc[qi], y[qi], rec);
                }
#pragma unroll
                for (int qi = 0; qi < Q; qi++) sel[qi].offer_keyed(IP ? -acc[qi] : acc[qi], pos0 + j, j < len && live[qi]);
            }
        }
    }

    // wave q joins the four waves' rows of query q
#pragma unroll
    for (int qi = 0; qi < Q; qi++) sel[qi].flush();
    __syncthreads();                                   // the tiles are no longer read
    u64* mb = reinterpret_cast<u64*>(smraw);           // [Q][4][k]
    const int k = a.k;
    constexpr uint32_t neg = IP ? 0x80000000u : 0u;
#pragma unroll
    for (int qi = 0; qi < Q; qi++) {
#pragma unroll
        for (int r = 0; r < KPL; r++) {
            const int e = r * 64 + lane;
            if (e < k) mb[(size_t)(qi * kSqfWaves + wave) * k + e] = sel[qi].best[r];
        }
    }
    __syncthreads();
#pragma unroll
    for (int qi = 0; qi < Q; qi++) {
        if (wave != qi || !live[qi]) continue;         // (wave-uniform)
        for (int w = 0; w < kSqfWaves; w++) {
            if (w == wave) continue;
            for (int e0 = 0; e0 < k; e0 += 64) {
                const int e = e0 + lane;
                const bool valid = e < k;
                sel[qi].offer_key(valid ? mb[(size_t)(qi * kSqfWaves + w) * k + e] : kMaxKey, valid);
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
            pq_emit<KPL>(sel[qi], k, neg, a.D + q * k, a.I + q * k, lane);
        }
    }
}

namespace {

// encode_vector (:446-455, :520-529) of x itself, IndexScalarQuantizer::add (:719-725): one wave per vector, lane l writes the
// code bytes l, l + 64, ...
__global__ __launch_bounds__(64) void sqflat_encode_kernel(const float* __restrict__ x, int d, const float* __restrict__ trained, int bits,
                                                           int uniform, int code_size, uint8_t* __restrict__ codes) {
    const int64_t v = blockIdx.x;
    uint8_t* code = codes + v * code_size;
    const float* xv = x + v * d;
    auto unit = [&](int i) {       // the component's place in [0, 1]
        const float vmin = uniform ? trained[0] : trained[i], vdiff = uniform ? trained[1] : trained[d + i];
        float xi = __fdiv_rn(__fsub_rn(xv[i], vmin), vdiff);
        if (xi < 0) xi = 0;
        if (xi > 1.0f) xi = 1.0f;
        return xi;
    };
    for (int b = threadIdx.x; b < code_size; b += 64) {
        if (bits == 8) {
            code[b] = (uint8_t)(int)__fmul_rn(255.f, unit(b));                      // :60
        } else {
            int c = (int)__dmul_rn((double)unit(2 * b), 15.0);                      // :88, a double multiply
            if (2 * b + 1 < d) c |= (int)__dmul_rn((double)unit(2 * b + 1), 15.0) << 4;
            code[b] = (uint8_t)c;
        }
    }
}

// decode_vector (:457-462, :531-536) of IndexScalarQuantizer::reconstruct_n (:789-797): the scalar codec, (c + 0.5f) / den by a
// true division whatever d is -- not the ORDER8 codec of the distances.  One thread per component.
__global__ __launch_bounds__(256) void sqflat_decode_kernel(const uint8_t* __restrict__ codes, int64_t n, int d, const float* __restrict__ trained,
                                                            int bits, int uniform, int code_size, float* __restrict__ x) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * d) return;
    const int64_t v = e / d;
    const int i = (int)(e - v * d);
    const uint8_t* code = codes + v * code_size;
    const uint32_t c = bits == 8 ? code[i] : (code[i >> 1] >> ((i & 1) << 2)) & 0xfu;
    const float vmin = uniform ? trained[0] : trained[i], vdiff = uniform ? trained[1] : trained[d + i];
    const float xi = __fdiv_rn(__fadd_rn((float)c, 0.5f), bits == 8 ? 255.f : 15.f);
    x[e] = __fadd_rn(vmin, __fmul_rn(xi, vdiff));
}

template <int Q, int KPL, bool IP, int BITS, bool UNIFORM, bool ORDER8>
void launch_sqf_i(const SqFlatScanArgs& a, const SqFlatPlan& P, int64_t tiles, hipStream_t s) {
    ensure_dynamic_lds(reinterpret_cast<const void*>(scan_sqflat_kernel<Q, KPL, IP, BITS, UNIFORM, ORDER8>), P.lay.bytes);
    hipLaunchKernelGGL((scan_sqflat_kernel<Q, KPL, IP, BITS, UNIFORM, ORDER8>), dim3((unsigned)tiles, (unsigned)P.S), dim3(256), P.lay.bytes, s, a,
                       P.lay, P.code_size, P.read == kSqReadTile128 ? 1 : 0);
}
template <int Q, int KPL, bool IP, int BITS, bool UNIFORM>
void launch_sqf_o(const SqFlatScanArgs& a, const SqFlatPlan& P, int64_t tiles, hipStream_t s) {
    if (P.order8) launch_sqf_i<Q, KPL, IP, BITS, UNIFORM, true>(a, P, tiles, s);
    else launch_sqf_i<Q, KPL, IP, BITS, UNIFORM, false>(a, P, tiles, s);
}
template <int Q, int KPL, bool IP>
void launch_sqf_t(const SqFlatScanArgs& a, const SqFlatPlan& P, int64_t tiles, hipStream_t s) {
    if (P.bits == 8) { if (P.uniform) launch_sqf_o<Q, KPL, IP, 8, true>(a, P, tiles, s); else launch_sqf_o<Q, KPL, IP, 8, false>(a, P, tiles, s); }
    else { if (P.uniform) launch_sqf_o<Q, KPL, IP, 4, true>(a, P, tiles, s); else launch_sqf_o<Q, KPL, IP, 4, false>(a, P, tiles, s); }
}
template <bool IP>
bool launch_sqf_k(const SqFlatScanArgs& a, const SqFlatPlan& P, int64_t tiles, hipStream_t s) {
    if (P.kpl == 16) {
        if (P.Q != 1) return false;
        launch_sqf_t<1, 16, IP>(a, P, tiles, s);
    } else if (P.kpl == 4) {
        if (P.Q == 1) launch_sqf_t<1, 4, IP>(a, P, tiles, s);
        else if (P.Q == 2) launch_sqf_t<2, 4, IP>(a, P, tiles, s);
        else launch_sqf_t<4, 4, IP>(a, P, tiles, s);
    } else {
        if (P.Q == 1) launch_sqf_t<1, 1, IP>(a, P, tiles, s);
        else if (P.Q == 2) launch_sqf_t<2, 1, IP>(a, P, tiles, s);
        else launch_sqf_t<4, 1, IP>(a, P, tiles, s);
    }
    return true;
}

}  // namespace

bool launch_scan_sqflat(const SqFlatScanArgs& a, const SqFlatPlan& P, bool inner_product, hipStream_t s) {
    if (a.nq <= 0) return true;
    if (!P.ok || a.S != P.S || a.slice_len != P.slice_len) return false;
    if (P.Q != 1 && P.Q != 2 && P.Q != 4) return false;
    if (P.read == kSqReadTile128 && (reinterpret_cast<uintptr_t>(a.codes) & 15u)) return false;
    if (P.order8 && (reinterpret_cast<uintptr_t>(a.codes) & 7u)) return false;
    const int64_t tiles = (a.nq + P.Q - 1) / P.Q;
    const bool ok = inner_product ? launch_sqf_k<true>(a, P, tiles, s) : launch_sqf_k<false>(a, P, tiles, s);
    if (!ok) return false;
    if (P.join) launch_join_rows(P.kpl, a.part, a.nq, a.S, (int64_t)a.S * a.k, a.k, inner_product ? 0x80000000u : 0u, a.D, a.I, nullptr, 0, s);
    return true;
}

void launch_sqflat_encode(const float* x, int64_t n, int d, const float* trained, int qtype, uint8_t* codes, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sqflat_encode_kernel, dim3((unsigned)n), dim3(64), 0, s, x, d, trained, sq_bits(qtype), sq_uniform(qtype) ? 1 : 0,
                       sq_code_size(d, qtype), codes);
}

void launch_sqflat_decode(const uint8_t* codes, int64_t n, int d, const float* trained, int qtype, float* x, hipStream_t s) {
    if (n <= 0) return;
    const int64_t e = n * d;
    hipLaunchKernelGGL(sqflat_decode_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, codes, n, d, trained, sq_bits(qtype),
                       sq_uniform(qtype) ? 1 : 0, sq_code_size(d, qtype), x);
}

}  // namespace vlq
